// sketch_rounds_kmer.inc -- phases 4 + 5 of a CLEAN wave of phi_sketch_winfix_kernel (every base ACGTacgt) when the graph has
// a k-mer table (PhiSketchArgs::k_rt): the wave's candidates on dense lanes, 64 per round, probed by their k-mer.  No
// MurmurHash3 here (DESIGN.md 4.1 "k-mer keys"):
//  - the walk-minimiser lookup only needs an injective key: phi_kmer_mix of the canonical k-mer, into a table of the read
//    table's bucket format whose ids are the same dense ids;
//  - every candidate is emitted: it is its read's first window, or the window minimum -- a k-mer -- changed, and two different
//    k-mers share a hash only by a MurmurHash3 collision, which the flush reports (PHI_KERR_HASH_COLLISION);
//  - a miss logs the K-MER; the wave tags its chunk (PHI_NOV_KMERS in nov_cnt) and phi_spectrum_flush_kernel hashes the entry,
//    once per read set.
// A wave with more novel k-mers than its chunk's log holds (rare, wave-uniform) sets `hashed`: the includer then runs the
// rounds of sketch_rounds.inc over the same items -- the probes find what they found, the log's entries are written again as
// hashes and the rest goes to the overflow list, which keeps holding hashes -- and leaves the chunk untagged.
// Items 1 .. ncand of s_meta (no predecessor item 0).  Included by sketch_win_fixed.hip; expects the names it declares.
    if (ncand > 0) {
        const ProbeArgs KP{A.k_rt, A.k_bmask, A.hit, A.err};
        const int cap = 1 << A.nov_shift;
        for (int r0 = 1; r0 <= ncand; r0 += 64) {
            const int t = r0 + lane;
            uint64_t v = 0;
            bool novel = false;
            if (t <= ncand) {
                v = SM((int)(s_meta[t] & 0x3FFu));
                novel = probe_table<false>(KP, phi_kmer_mix(v));
            }
            // the round's novel k-mers, appended to the chunk's log in lane order: one coalesced store
            const unsigned long long ib = __ballot(novel);
            const int pos = n_log + __popcll(ib & ((1ull << lane) - 1));
            if (novel && pos < cap) A.nov_log[((A.log_base + chunk) << A.nov_shift) + pos] = v;
            n_log += __popcll(ib);
        }
        n_emit = ncand;
        if (n_log > cap) {
            hashed = true;
            n_log = 0; n_emit = 0;
            if (lane == 0) s_meta[0] = (MetaT)ITEM_NOEMIT;    // (item 1 is its read's first window: the item before it only has to exist)
            wave_sync();
        }
    }

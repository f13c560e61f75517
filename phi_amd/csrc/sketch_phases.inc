// sketch_phases.inc -- phases 0 .. 3b of the base-space sketch kernels: staging of a chunk, canonical k-mers, window
// minima, read starts, candidate flags, items.  Included in the body of phi_sketch_kernel (sketch.hip: one chunk per
// wave) and of phi_sketch_pool_kernel (sketch_pooled.hip: a wave takes several chunks of a read batch): the text is the
// same, the kernels differ in what surrounds it.  Expects the names both kernels declare before the #include, and
// sketch_dev.h.
    // ---- phase 0: stage the chunk's packed words and bitmaps (the only global reads up to the
    //      output phase).  Local base lb <-> base c0-32+lb; local bit lp <-> base c0-64+lp.
    unsigned long long my_bad = 0;
    StartProbe probe{};
    if (FUSED) {
        // straight from ASCII: lane -> 16 bases = one 32-bit half of a packed word + 16 flags of bases outside ACGTacgt
        uint32_t x[4];
        if (POOL) {
            // this chunk's bases were asked for a turn ago; ask for the next chunk's now: the load travels under this
            // turn's arithmetic (the waves of a SIMD run their turns nearly in step -- a load at the top of a turn finds
            // no other wave to hide behind)
            x[0] = xn.x; x[1] = xn.y; x[2] = xn.z; x[3] = xn.w;
            if (ci + 1 < mine) xn = load_bases16(A.ascii, N, c0 + stride * WCH, lane);
        } else {
            const uint4 v = load_bases16(A.ascii, N, c0, lane);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        }
        if (!A.uniform_len) probe = start_probe_issue(A, c0, lane);   // the first probe of the read-start search travels with the bases
        uint32_t code = 0, bad = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t t = ((x[q] >> 1) ^ (x[q] >> 2)) & 0x03030303u;      // 2-bit code of each byte
            const uint32_t c8 = (t * 0x40100401u) >> 24;                        // the four codes, first base on top
            code = (code << 8) | c8;
            // spelled back from the per-byte codes (one byte lookup: no gather needed) against the upper-cased bytes
            if (__builtin_amdgcn_perm(0x54474341u, 0x54474341u, t) != (x[q] & 0xDFDFDFDFu)) {   // a byte outside ACGTacgt (rare)
#pragma unroll
                for (int j = 0; j < 4; j++) bad |= (uint32_t)(!phi_is_acgt((x[q] >> (8 * j)) & 0xFFu)) << (4 * q + j);
            }
        }
        reinterpret_cast<uint32_t *>(s_words)[lane ^ 1] = code;                 // word = (even lane's half << 32) | odd lane's
        uint16_t *s_bad16 = reinterpret_cast<uint16_t *>(s_bad);
        if (lane < 62) s_bad16[lane + 2] = (uint16_t)bad;                       // bit of base b+j = 32 + 16 lane + j
        else { s_bad16[lane - 62] = 0; bad = 0; }                               // bases before c0-32 / past c0+960 are never looked at
        if (lane < SBW) s_bits[lane] = 0;
        my_bad = bad;
    } else {
        const int64_t n_words = (N + 31) / 32 + 2;        // the buffer carries two zero padding words
        const int64_t n_sw = N / 64 + 2;
        if (lane < SWW) {
            const int64_t wi = (c0 >> 5) - 1 + lane;
            s_words[lane] = (wi >= 0 && wi < n_words) ? A.words[wi] : 0;
        } else if (lane - SWW < SBW) {
            const int64_t wi = (c0 >> 6) - 1 + (lane - SWW);
            s_bits[lane - SWW] = (wi >= 0 && wi < n_sw) ? A.starts[wi] : 0;
        } else {
            const int64_t wi = (c0 >> 6) - 1 + (lane - SWW - SBW);
            if (have_bad) my_bad = (wi >= 0 && wi < n_sw) ? A.badbits[wi] : 0;
            s_bad[lane - SWW - SBW] = my_bad;
        }
    }
    chunk_bad = have_bad && __ballot(my_bad != 0) != 0ull;   // wave-uniform
    wave_sync();

    if (MODE == PHI_MODE_WRITE) out_base = A.block_off[chunk];

#if PHI_ABL == 10
    return;
#endif
    if (FUSED && KT < 0) {
        // k > 32 (an instantiation of its own: KT = -1): no 2-bit k-mers; every window of the chunk takes the exact byte-wise routine
        // (its novel hashes go to the overflow list, the chunk's own log stays empty)
        if (A.uniform_len) start_bits_uniform(A, c0, lane, s_bits);
        else start_bits_from_offsets(A, c0, lane, probe, s_bits);
        wave_sync();
        int n_emit_slow = 0, n_nov = 0;
        slow_windows<MODE, true>(A, c0, chunk, lane, k, w, s_bits, s_bad, true, 0, n_emit_slow, n_nov);
        if (A.q_clean) clean_finish(A, chunk, (int64_t)gridDim.x * (TPB / 64), lane);
        if (lane == 0) {
            A.nov_cnt[A.log_base + chunk] = 0;
            const int stripe = (int)(chunk & (PHI_STRIPES - 1)) * 8;
            if (n_nov && A.n_logged) atomicAdd(A.n_logged + stripe, (unsigned long long)n_nov);
            if (n_emit_slow && A.n_emitted) atomicAdd(A.n_emitted + stripe, (unsigned long long)n_emit_slow);
        }
        return;
    }
    // ---- phase 1: canonical k-mers, P consecutive per lane
    {
        const int P = KT > 0 ? (WCH + WT + 63) / 64 : (M + 63) / 64;
        const int l0 = lane * P;
        if (c0 >= 1 && c0 - 1 + (int64_t)P * 64 + k <= N) {
            // interior chunk (all but the first and last of a batch): every k-mer a lane touches
            // exists, so the roll needs no per-position checks, and every lane stores all P of its
            // k-mers (the slots past M are spare).  Slot of l0+i: a0 + i + carry of (l0 & 7) + i.
            // (the last lanes, whose k-mers nobody reads, sit the roll out: one branch around all of it)
            if (l0 < M) {
                uint64_t F = lds_extract64(s_words, l0 + 31) >> (64 - 2 * k);
                uint64_t R = phi_revcomp(F, k);
                uint64_t nxt = lds_extract64(s_words, l0 + 31 + k);     // bases j+k .. j+k+31
                uint64_t *s_p = s_mp + l0 + (l0 >> 3);
                const int lo7 = l0 & 7;
#pragma unroll
                for (int i = 0; i < P; i++) {
                    if (i) {
                        const uint64_t b = nxt >> 62;
                        nxt <<= 2;
                        F = ((F << 2) | b) & kmask;
                        R = (R >> 2) | ((3 - b) << (2 * k - 2));
                    }
#if PHI_ABL == 3
                    if (i == 0)
#endif
                    s_p[i + ((lo7 + i) >> 3)] = FMIN ? min_u62(F, R) : (F < R ? F : R);
                }
            }
        } else {
            const int l1 = min(l0 + P, M);
            const int64_t j0 = c0 - 1 + l0;
            uint64_t F = 0, R = 0, nxt = 0;
            bool live = false;
            for (int l = l0; l < l1; l++) {
                const int64_t j = j0 + (l - l0);
                uint64_t m = ~0ull;
                if (j >= 0 && j + k <= N) {
                    if (!live) {
                        F = lds_extract64(s_words, l + 31) >> (64 - 2 * k);
                        R = phi_revcomp(F, k);
                        nxt = lds_extract64(s_words, l + 31 + k);   // bases j+k .. j+k+31
                        live = true;
                    } else {
                        const uint64_t b = nxt >> 62;
                        nxt <<= 2;
                        F = ((F << 2) | b) & kmask;
                        R = (R >> 2) | ((3 - b) << (2 * k - 2));
                    }
                    m = F < R ? F : R;
                }
                SM(l) = m;
            }
        }
    }
    wave_sync();

#if PHI_ABL == 11
    return;
#endif
#include "sketch_minima.inc"

#if PHI_ABL == 12
    { uint64_t acc = 0;
#pragma unroll
      for (int i = 0; i <= Q; i++) acc ^= wv[i] + (uint64_t)i;
      asm volatile("" :: "v"(acc)); return; }
#endif
    if (FUSED) {
        // the read starts inside this chunk's base range, from the read offsets (answer of the probe issued in phase 0)
        if (A.uniform_len) start_bits_uniform(A, c0, lane, s_bits);
        else start_bits_from_offsets(A, c0, lane, probe, s_bits);
        wave_sync();
    }
#if PHI_ABL == 13
    { uint64_t acc = 0;
#pragma unroll
      for (int i = 0; i <= Q; i++) acc ^= wv[i] + (uint64_t)i;
      asm volatile("" :: "v"(acc)); return; }
#endif
    // ---- phase 3: candidate windows of this lane: outputs i = 1..Q, window start a = c0-1+lane*Q+i
    //      (local bit of base a = la + 63 with la = lane*Q + i)
    uint32_t cflag = 0, fflag = 0, pflag = 0;             // candidates; first windows; candidates that carry their predecessor
    {
        const int64_t a0 = c0 - 1 + (int64_t)lane * Q;
        const int lp0 = lane * Q + 63;                    // local bit of base a0
        // windows a0+i with i <= imax end inside the batch
        const int64_t room = N - span - a0;
        const int imax = room > Q ? Q : (int)room;
        if (span <= 64 - Q) {
            // sb bit j <-> base a0+1+j: one funnel shift serves all Q windows of this lane
            const int lb = lp0 + 1;
            const int wi = lb >> 6, sh = lb & 63;
            const unsigned long long lo = s_bits[wi];
            const unsigned long long sb = sh ? (lo >> sh) | (s_bits[wi + 1] << (64 - sh)) : lo;
            // bb bit j <-> base a0+j is outside ACGT: window a and its predecessor cover a-1 .. a+span-1
            unsigned long long bb = 0;
            if (chunk_bad) {
                const int wj = lp0 >> 6, sj = lp0 & 63;
                const unsigned long long lo2 = s_bad[wj];
                bb = sj ? (lo2 >> sj) | (s_bad[wj + 1] << (64 - sj)) : lo2;
            }
            // bit i of `blocked`: some sequence starts at bases a+1 .. a+span-1 of window i, i.e. sb has a
            // bit in [i, i+span-2]: OR over a sliding range by doubling (1,2,4,...,32, then the rest)
            unsigned long long t = sb;
            t |= t >> 1; t |= t >> 2; t |= t >> 4; t |= t >> 8; t |= t >> 16;     // ranges of 32
            const int len1 = span - 1;                                              // 1 .. 55
            unsigned long long blocked;
            if (len1 >= 32) blocked = t | (t >> (len1 - 32));
            else {
                // shorter ranges: rebuild from the powers of two below len1
                unsigned long long u = sb, acc = 0;
                int have = 0;
                for (int b = 0; b < 5; b++) {
                    if (len1 & (1 << b)) { acc |= u >> have; have += 1 << b; }
                    u |= u >> (1 << b);
                }
                blocked = len1 > 0 ? acc : 0ull;
            }
            // bit i of `dirty`: a base outside ACGT under window i or its predecessor: bb bit in [i-1, i+span-1]
            unsigned long long dirty = 0;
            if (chunk_bad) {
                unsigned long long v = bb;
                v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
                const int len2 = span + 1;                                          // 2 .. 57
                if (len2 >= 32) v = v | (v >> (len2 - 32));
                else {
                    unsigned long long u = bb, acc = 0;
                    int have = 0;
                    for (int b = 0; b < 5; b++) {
                        if (len2 & (1 << b)) { acc |= u >> have; have += 1 << b; }
                        u |= u >> (1 << b);
                    }
                    v = acc;
                }
                dirty = v << 1;                                                     // bit i <-> range starting at i-1
            }
            uint32_t changed = 0;
#pragma unroll
            for (int i = 1; i <= Q; i++) changed |= (uint32_t)(wv[i] != wv[i - 1]) << i;
            const uint32_t first = ((uint32_t)sb & ((1u << Q) - 1)) << 1;           // bit i <-> sb bit i-1
            const uint32_t in_batch = imax >= 1 ? ((2u << imax) - 2u) : 0u;        // bits 1 .. imax
            // the first window after a stretch left to the byte-wise path: the candidate before it is not its
            // predecessor window, so it becomes a candidate that carries its own predecessor (whose value
            // is valid: a window that is not dirty has no such base under its predecessor either)
            uint32_t reseed = 0;
            if (chunk_bad) {
                const uint32_t dall = (uint32_t)dirty | (uint32_t)range_has_bit(s_bad, lp0 - 1, lp0 + span - 1);   // bit 0: window 0
                reseed = ~dall & (dall << 1);
            }
            cflag = in_batch & ~(uint32_t)blocked & ~(uint32_t)dirty & (first | changed | reseed) & ((2u << Q) - 2u);
            fflag = cflag & first;
            pflag = cflag & reseed & ~first;
        } else {
            const int lim = lp0 + Q + span + 1;
            int ns = next_start_lds(s_bits, lp0 + 2, lim);
#pragma unroll
            for (int i = 1; i <= Q; i++) {
                const int lp = lp0 + i;
                if (ns <= lp) ns = next_start_lds(s_bits, lp + 1, lim);
                bool valid = (i <= imax) && (ns > lp + span - 1);
                if (valid && chunk_bad) valid = !range_has_bit(s_bad, lp - 1, lp + span - 1);
                if (valid) {
                    const bool first = (s_bits[lp >> 6] >> (lp & 63)) & 1ull;
                    const bool reseed = chunk_bad && !first && range_has_bit(s_bad, lp - 2, lp + span - 2);   // the window before is byte-wise
                    if (first || reseed || wv[i] != wv[i - 1]) {
                        cflag |= 1u << i;
                        if (first) fflag |= 1u << i;
                        if (reseed) pflag |= 1u << i;
                    }
                }
            }
        }
    }
#if PHI_ABL == 14
    { uint64_t acc = cflag ^ (fflag << 9) ^ ((uint64_t)pflag << 20);
#pragma unroll
      for (int i = 0; i <= Q; i++) acc ^= wv[i] + (uint64_t)i;
      asm volatile("" :: "v"(acc)); return; }
#endif
    // wave prefix sum of the per-lane candidate counts
    int coff;
    {
        const int cnt = __popc(cflag) + __popc(pflag);
        const int v = wave_scan_inclusive(cnt);
        ncand = __builtin_amdgcn_readlane(v, 63);
        coff = v - cnt;
    }
    wave_sync();                                          // every lane has read its k-mers
    {
        // the minimum of window slot s = lane*Q + i goes to SM(s) (constant offsets again); slot 0 is
        // the window before the chunk's first
        if (lane == 0) s_q[0] = wv[0];
#pragma unroll
        for (int i = 1; i <= Q; i++) SQ(i) = wv[i];
        // item list: item 0 = the window before the chunk's first candidate (only its hash is needed),
        // item 1 + c = candidate c.  Every lane stores all Q windows, the non-candidates into trash
        // slots past the last item: no divergent branch per window
        int c = coff + 1;
        const int trash = phi_wave_items(w, k) + (lane & 3);
        if (!chunk_bad && !NEED_POS) {
            // a lane has 0.6 candidates on average, rarely more than three: a loop over the set bits issues fewer
            // instructions than eight predicated stores
            for (uint32_t f = cflag; f; f &= f - 1) {
                const uint32_t i = (uint32_t)__ffs((int)f) - 1;
                s_meta[c++] = (MetaT)((uint32_t)(lane * Q) + i + (((fflag >> i) & 1u) ? ITEM_FIRST : 0u));
            }
        } else if (!chunk_bad) {
#pragma unroll
            for (int i = 1; i <= Q; i++) {
                const bool on = (cflag >> i) & 1u;
                s_meta[on ? c : trash] = (MetaT)((uint32_t)(lane * Q + i) | (NEED_POS ? (uint32_t)wp[i] << 10 : 0u) | (((fflag >> i) & 1u) ? ITEM_FIRST : 0u));
                c += on;
            }
        } else {
            // (rare) a candidate after a byte-wise stretch is preceded by the window before it
#pragma unroll
            for (int i = 1; i <= Q; i++) {
                if ((cflag >> i) & 1u) {
                    if ((pflag >> i) & 1u) s_meta[c++] = (MetaT)((uint32_t)(lane * Q + i - 1) | ITEM_NOEMIT);
                    s_meta[c++] = (MetaT)((uint32_t)(lane * Q + i) | (NEED_POS ? (uint32_t)wp[i] << 10 : 0u) | (((fflag >> i) & 1u) ? ITEM_FIRST : 0u));
                }
            }
        }
        if (coff == 0 && cflag) s_meta[0] = (MetaT)((uint32_t)(lane * Q + __ffs((int)cflag) - 2) | ITEM_NOEMIT);
    }
    wave_sync();
#undef SQ

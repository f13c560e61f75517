// sketch_rounds.inc -- phases 4 + 5 of the one-wave-per-chunk sketch kernels: the chunk's items on dense
// lanes, 64 per round -- murmur3 of the item's minimum, the hash-change test against the item before it (the lane below;
// lane 0 takes the last lane of the round before), ordered compaction, output.  Included by phi_sketch_kernel and
// phi_sketch_win_kernel (sketch.hip) and by phi_sketch_winfix_kernel (sketch_win_fixed.hip); expects the names they
// declare before the #include.
    if (ncand > 0) {
        uint64_t carry = PHI_EMPTY_KEY;
        for (int r0 = 0; r0 <= ncand; r0 += 64) {
            const int t = r0 + lane;
            const bool valid = t <= ncand;
            uint32_t meta = 0;
            uint64_t h = 0;
            if (valid) {
                meta = s_meta[t];
                h = phi_kmer_hash(SM((int)(meta & 0x3FFu)), k);
            }
            const uint64_t hp = wave_prev_u64(h, carry, lane);
            carry = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(h >> 32), 63) << 32) |
                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h, 63);
            const bool emit = valid && !(meta & ITEM_NOEMIT) && ((meta & ITEM_FIRST) || h != hp);
            const unsigned long long bal = __ballot(emit);
            bool novel = false;
            if (emit) {
                const int rank = n_emit + __popcll(bal & ((1ull << lane) - 1));
                if (MODE == PHI_MODE_WRITE) {
                    A.out_hash[out_base + rank] = h;
                    A.out_pos[out_base + rank] = c0 - 1 + (int64_t)((meta >> 10) & 0x3FFu);
                } else if (MODE == PHI_MODE_PROBE) {
                    novel = probe_table(A, h);
                }
            }
            if (MODE == PHI_MODE_PROBE) {
                // the round's novel hashes, appended to the chunk's log in lane order: one coalesced store
                const unsigned long long ib = __ballot(novel);
                const int pos = n_log + __popcll(ib & ((1ull << lane) - 1));
                const int cap = 1 << A.nov_shift;
                if (novel && pos < cap) A.nov_log[((A.log_base + chunk) << A.nov_shift) + pos] = h;
                n_log += __popcll(ib);
                if (n_log > cap) {                            // (wave-uniform, rare) past the chunk's log: the overflow list
                    const OverflowArgs O{A.ov_list, A.ov_count, A.ov_cap, A.err};
                    overflow_novel(O, novel && pos >= cap, h, lane);
                }
            }
            n_emit += __popcll(bal);
        }
    }

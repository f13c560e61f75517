// sketch_minima.inc -- phase 2 of the sketch kernels: the minima of the Q + 1 windows of a lane from the
// k-mers at s_q.  Included by sketch_phases.inc (base positions) and by phi_sketch_win_kernel (sketch.hip) and
// phi_sketch_winfix_kernel (sketch_win_fixed.hip; windows of reads of one length): the two differ in where a lane's
// k-mers lie, not in how their minima are taken.  Defines SQ, wv and wp.
    // ---- phase 2: minima of windows la = lane*Q .. lane*Q+Q  (window la = m[la .. la+w)); the
    //      k-mer of slot lane*Q + x is s_q[x + (x >> 3)]: constant offsets from one address
#define SQ(x) s_q[(x) + ((x) >> 3)]
    uint64_t wv[Q + 1];
    int wp[Q + 1];
    {
        const int base = lane * Q;
        if (WIDE && FMIN) {
            // values only (no positions): the rightmost-tie rule does not change a minimum's value
            uint64_t L[Q];                        // L[i] = min of m[base+i .. base+Q)
            L[Q - 1] = SQ(Q - 1);
#pragma unroll
            for (int i = Q - 2; i >= 0; i--) L[i] = min_u62(SQ(i), L[i + 1]);
            uint64_t core = SQ(Q);
#if PHI_ABL != 1
#pragma unroll
            for (int x = Q + 1; x < WT; x++) core = min_u62(core, SQ(x));
#endif
            uint64_t Rr = 0;                      // min of m[base+w .. base+w+i)
#pragma unroll
            for (int i = 0; i <= Q; i++) {
                uint64_t t = (i < Q) ? min_u62(L[i], core) : core;
                if (i > 0) {
                    const uint64_t e = SQ(WT + i - 1);
                    Rr = (i == 1) ? e : min_u62(Rr, e);
                    t = min_u62(t, Rr);
                }
                wv[i] = t; wp[i] = 0;
            }
        } else if (WIDE) {
            MinEnt L[Q + 1];                      // L[i] = min of m[base+i .. base+Q), ties right
            L[Q].v = 0; L[Q].i = -1;
#pragma unroll
            for (int i = Q - 1; i >= 0; i--) {
                MinEnt e; e.v = SQ(i); e.i = NEED_POS ? base + i : 0;
                L[i] = (i == Q - 1) ? e : take_right(e, L[i + 1]);
            }
            MinEnt core; core.v = SQ(Q); core.i = NEED_POS ? base + Q : 0;
            for (int x = Q + 1; x < w; x++) {
                MinEnt e; e.v = SQ(x); e.i = NEED_POS ? base + x : 0;
                core = take_right(core, e);
            }
            MinEnt Rr; Rr.v = 0; Rr.i = -1;       // min of m[base+w .. base+w+i)
#pragma unroll
            for (int i = 0; i <= Q; i++) {
                MinEnt t = (i < Q) ? take_right(L[i], core) : core;
                if (i > 0) {
                    MinEnt e; e.v = SQ(w + i - 1); e.i = NEED_POS ? base + w + i - 1 : 0;
                    Rr = (i == 1) ? e : take_right(Rr, e);
                    t = take_right(t, Rr);
                }
                wv[i] = t.v; wp[i] = t.i;
            }
        } else {
#pragma unroll
            for (int i = 0; i <= Q; i++) {
                MinEnt t; t.v = SQ(i); t.i = NEED_POS ? base + i : 0;
                for (int x = 1; x < w; x++) {
                    MinEnt e; e.v = SQ(i + x); e.i = NEED_POS ? base + i + x : 0;
                    t = take_right(t, e);
                }
                wv[i] = t.v; wp[i] = t.i;
            }
        }
    }

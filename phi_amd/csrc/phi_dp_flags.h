// phi_dp_flags.h -- the flag bits of word 0 of a DP step record, shared by the kernels that read the records (dp.hip,
// dp_events.hip, through phi_kernels.h) and the plain host code that writes them (dp_steps.h), and the DP's constants
// that the solve's plain host code (solve_host.h) shares with the kernels.  No HIP include.
// The record layout itself is documented at PhiDpArgs / PhiDpEventArgs of phi_kernels.h.
#pragma once

#define PHI_DP_NEED_ENTRY 1     // step flag: a recombination can enter this vertex
#define PHI_DP_NEED_TOPS 2      // step flag: a recombination can leave this vertex
#define PHI_DP_LANE_ONLY 4      // compact-step flag: a walk starts or ends on the vertex (no ENTRY / TOPS work)
#define PHI_DP_PAIR 8           // compact-step flag: this step and the next have no TOPS and no walk in common
                                // (two alleles of one site): the consumer may take them in one iteration

#define PHI_RCAP 32             // DP run-length states 0..31 (an anchor spans <= k-1 <= 31 edges)
#define PHI_DP_BLOCK_MAX 2048   // steps of a block at most (= the larger ring of tops)
#define PHI_DP_NEGK (-(1 << 30))   // "no run" in key space

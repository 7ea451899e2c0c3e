// Pieces of the variational lower bound of a DBN (mdbn_bound.hip): the fused propdown + row log-likelihood and the replica
// sampler.  Arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "philox.h"

namespace mdbn {

constexpr int ROWLL_BM = 128;               // replica rows of a tile
constexpr int ROWLL_BN = 128;               // visible columns of a tile
constexpr int ROWLL_BK = 32;                // hidden units of a K stage
constexpr int ROWLL_NT = 256;               // threads: four waves, 64 x 64 of the tile each

// out[r] = log p(target[r / target_div] | h[r]) under sigmoid / unit-variance Gaussian visibles.
// PRECONDITION: h holds 0 / 1 only (it enters the matrix pipe as ONE bf16 piece: any other value is truncated to its upper
// 16 bits).  The padding of h and W beyond H, and of target beyond V, is never used.
struct RowllArgs {
    int R, V, H, gauss;
    int target_div;                          // >= 1: replica row r is scored against target row r / target_div
    int tiles_m, tiles_n;                    // ceil(R / ROWLL_BM), ceil(V / ROWLL_BN)
    int64_t ldh, ldv;                        // leading dimensions of h and W (ldh), of target (ldv)
    const float* h; const float* W;          // [R][ldh] 0 / 1 samples; [V][ldh]
    const float* vbias; const float* target; // [V]; [ceil(R / target_div)][ldv]
    float* partial;                          // [tiles_n][R]: the row sums of one column tile each
    float* out;                              // [R]
};

// The same call for a layer whose visible columns [span_lo, span_hi) are softmax groups (table: include/mdbn_hip.h,
// "Categorical visible units"): a group adds sum_c t_c pre_c - logsumexp_c pre_c, a column outside the span the Bernoulli term.
// a.gauss = 0.  a.partial holds ROWLL_GP floats per (column tile, row): [tiles_n][ROWLL_GP][R] -- the tile's sum of everything
// that is complete inside it, then (max, sum of exp(pre - max)) of the HEAD fragment (a group that began in the previous tile)
// and of the TAIL fragment (a group that continues in the next one); a sum of 0 says "no such fragment".
constexpr int ROWLL_GP = 5;
struct RowllGroupArgs {
    RowllArgs a;
    const int32_t* group_start;              // device copy [n_groups + 1]; every value read is clamped to [span_lo, span_hi]
    int n_groups;                            // >= 1
    int span_lo, span_hi;                    // group_start_host[0], group_start_host[n_groups]: checked by the caller
};

struct ReplicaArgs {
    int64_t N, S, H, ldh;                    // data rows, replicas per row, live / stored columns
    const float* mean;                       // [N][ldh]
    float* sample;                           // [N S][ldh]: row n S + s = (u[n S + s] < mean[n]); pad columns 0
    float* entropy;                          // [N] or NULL: -sum_j m log m + (1 - m) log(1 - m), 0 log 0 = 0
    PhiloxKey rng;                           // the addressing of mdbn_rng_uniform(rows = N S, cols = H)
};

inline int64_t rowll_partial_floats(int64_t R, int64_t V) { return ((V + ROWLL_BN - 1) / ROWLL_BN) * R; }
inline int64_t rowll_grouped_partial_floats(int64_t R, int64_t V) { return ROWLL_GP * rowll_partial_floats(R, V); }
hipError_t launch_rowll(const RowllArgs& a, hipStream_t s);
hipError_t launch_rowll_grouped(const RowllGroupArgs& g, hipStream_t s);
hipError_t launch_sample_replicas(const ReplicaArgs& a, hipStream_t s);

}  // namespace mdbn

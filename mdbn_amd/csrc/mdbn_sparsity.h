// Sparsity target for the hidden units (mdbn_sparsity.hip): the running estimate of every unit's mean activation and the
// penalty's additions to the packed statistics [S | s_h | s_v | cost].  Arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdbn {

constexpr int SPARSITY_NT = 256;            // threads of a sparsity_stats workgroup

// q += rate (mean_r ph[r] - q), v_mean = mean_r v0[r]; the rows of a column summed in ascending order (compensated)
struct SparsityActivityArgs {
    const float* ph; const float* v0;       // [B][ldh], [B][ldv] (v0 null: the hidden half only)
    int64_t ldh, ldv;
    int B, V, H;
    float rate;                             // in (0, 1]; 1: q becomes the batch mean exactly
    float* q; float* v_mean;                // [H], [V] (null with v0)
};

// with t_j = target - q_j: S_ij = fmaf(w_scale v_mean[i], t_j, S_ij) in place, s_h[j] = fmaf(b_scale, t_j, s_h[j])
struct SparsityStatsArgs {
    float* stats;                           // packed [V ldh | ldh | ldv | 4]
    int64_t ldh;
    int V, H;
    int rows;                               // rows of S a workgroup owns (center_rows_per_block)
    const float* q; const float* v_mean;    // [H], [V] (v_mean is not read with w_scale = 0)
    float target, w_scale, b_scale;         // w_scale = 0: S is not touched; b_scale = 0: s_h is not touched
};

hipError_t launch_sparsity_activity(const SparsityActivityArgs& a, hipStream_t s);
hipError_t launch_sparsity_stats(const SparsityStatsArgs& a, hipStream_t s);

}  // namespace mdbn

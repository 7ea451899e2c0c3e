// Learned per-column variance of a Gaussian visible layer (mdbn_sigma.hip): the rows of a minibatch scaled by
// exp(+-log_sigma) on their way into (and out of) the unit-variance model, and the exact gradient step of log_sigma from the
// rows in units and their conditional means.  Arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdbn {

constexpr int SIGMA_NT = 256;               // threads of a sigma_scale_rows workgroup: 256 groups of four columns side by side
constexpr int SIGMA_STAT_NT = 64;           // threads of a sigma_update workgroup: one wave, four columns per thread
constexpr int SIGMA_ONE_STAGE_ROWS = 64;    // up to this many rows a workgroup walks all of them and finishes in the same launch
constexpr int SIGMA_SLICE_ROWS = 16;        // above: rows of one partial sum (stage 1), the partials finished in ascending order

// dst[r, i] = src[idx[r], i] * expf(sign * log_sigma[i]) for i < V, 0 for V <= i < ld_dst
struct SigmaScaleArgs {
    const float* src; int64_t n_src, ld_src;        // [n_src][ld_src]; columns V.. are not read
    const void* idx; int idx64;                     // [B] int32 / int64 rows of src (negative: from the end; clamped), or null: row r
    int B, V;
    const float* log_sigma;                         // [V]
    float sign;                                     // -1: raw rows to units, +1: units back to raw
    float* dst; int64_t ld_dst;                     // [B][ld_dst]
    int rows_per_block;                             // a multiple of 4
};

// q_i = sum_{r < n_rows} U_ri (U_ri - M_ri), g_i = q_i / n_rows - 1, then the bias rule on log_sigma with the OLD speed:
// s_i = clamp(s_i + speed_i lr, lo, hi), speed_i = g_i + (speed_i - g_i) momentum
struct SigmaUpdateArgs {
    const float* U; const float* M;                 // [n_rows][ldu], [n_rows][ldm]; columns V.. are not read
    int64_t ldu, ldm;
    int n_rows, V;
    int n_slices;                                   // 1: one stage
    float lr, momentum, lo, hi;
    float* log_sigma; float* speed;                 // [V], in place
    float* partials;                                // [n_slices][ru4(V)] (two stages)
};

inline int sigma_slices(int64_t rows) { return rows <= SIGMA_ONE_STAGE_ROWS ? 1 : (int)((rows + SIGMA_SLICE_ROWS - 1) / SIGMA_SLICE_ROWS); }

hipError_t launch_sigma_scale_rows(SigmaScaleArgs a, hipStream_t s);
hipError_t launch_sigma_update(const SigmaUpdateArgs& a, hipStream_t s);

}  // namespace mdbn

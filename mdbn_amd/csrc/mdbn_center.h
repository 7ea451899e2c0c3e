// Centred CD training (mdbn_center.hip): the running offsets of the visible and hidden units and the offset correction of
// the packed statistics [S | s_h | s_v | cost].  Arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdbn {

constexpr int CENTER_NT = 256;              // threads of a center_stats workgroup
constexpr int CENTER_MAXCH = 4;             // 16-byte column groups one thread of it owns in a row
constexpr int CENTER_MAX_H = 4 * CENTER_NT * CENTER_MAXCH;     // widest S the kernel serves (4096 hidden units)
constexpr int CENTER_OFF_NT = 64;           // threads of a center_offsets workgroup (one column each)

// mu += nu (mean_r v0[r] - mu), lam += nu (mean_r ph[r] - lam); the rows of a column summed in ascending order (compensated)
struct CenterOffsetsArgs {
    const float* v0; const float* ph;       // [B][ldv], [B][ldh]
    int64_t ldv, ldh;
    int B, V, H;
    float nu;                               // in (0, 1]; 1: the offsets become the batch means exactly
    float* mu; float* lam;                  // [V], [H]
};

// S'_ij = S_ij - mu_i s_h[j] - s_v[i] lam_j in place, s_v'[i] = s_v[i] - rho sum_j S'_ij lam_j, the row blocks' partial
// sums sum_{i in block} mu_i S'_ij in `partial`; then (center_finish_kernel) s_h'[j] = s_h[j] - rho sum_blocks partial
struct CenterStatsArgs {
    float* stats;                           // packed [V ldh | ldh | ldv | 4]
    int64_t ldv, ldh;
    int V, H;
    int rows;                               // rows of S a workgroup owns (center_rows_per_block)
    int blocks;                             // ceil(V / rows)
    int ldp;                                // floats per row of `partial`: round_up(H, 4)
    float rho;
    const float* mu; const float* lam;      // [V], [H]
    float* partial;                         // [blocks][ldp]
};

// Rows of S per workgroup: a multiple of 8, as many as leave at least two workgroups per CU of a 256-CU part (every
// block's partial column sums are written and read once more: 2 / rows of the traffic of S itself)
inline int center_rows_per_block(int64_t V) { return V >= 32 * 512 ? 32 : V >= 16 * 512 ? 16 : 8; }
inline int64_t center_blocks(int64_t V) { const int r = center_rows_per_block(V); return (V + r - 1) / r; }
inline int64_t center_partial_floats(int64_t V, int64_t H) { return center_blocks(V) * ((H + 3) & ~int64_t(3)); }

hipError_t launch_center_offsets(const CenterOffsetsArgs& a, hipStream_t s);
hipError_t launch_center_stats(const CenterStatsArgs& a, hipStream_t s);

}  // namespace mdbn

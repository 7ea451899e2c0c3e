// Absent visible units (mdbn_absent.hip): training on rows with missing entries after Salakhutdinov, Mnih & Hinton 2007 -- a
// visible unit a row did not observe (NaN in the table) is absent from that row's RBM; all rows share one set of weights.
// Arguments and launchers of the four row kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "philox.h"

namespace mdbn {

constexpr int ABSENT_NT = 256;              // threads of a workgroup: 256 columns (8 mask words) of one row / one 4-row block

// mask words of one row: bit (i & 31) of word (i >> 5) is set when column i is observed; bits of columns >= V are 0
inline int64_t absent_words(int64_t V) { return (V + 31) / 32; }
inline int64_t absent_col_blocks(int64_t V) { return (V + ABSENT_NT - 1) / ABSENT_NT; }
// workgroups of absent_split (one row each) and of absent_visible (one 4-row block each: = its cost partials)
inline int64_t absent_split_blocks(int64_t B, int64_t V) { return absent_col_blocks(V) * B; }
inline int64_t absent_visible_blocks(int64_t B, int64_t V) { return absent_col_blocks(V) * ((B + 3) / 4); }

struct AbsentSplitArgs {
    const float* x; int64_t ldx;            // [B][ldx], NaN = missing in columns < V (pad columns are not read)
    float* filled; int64_t ld_filled;       // [B][ld_filled]: x with 0 where missing; may be x itself
    uint32_t* observed;                     // [B][absent_words(V)]
    int32_t* row_count;                     // [B] observed entries of the row; nullable
    int B, V;
};
hipError_t launch_absent_split(const AbsentSplitArgs& a, hipStream_t s);

struct AbsentVisibleArgs {
    const float* pre;                       // [B][ld] linear pre-activations h W^T + vbias
    float* mean; float* sample; float* tap; // [B][ld] each, nullable; mean may be `pre` itself
    const float* v0; float* cost_partials;  // zero-filled cost target and one partial per workgroup (both or neither)
    const uint32_t* observed;               // [B][absent_words(V)]
    int B, V;
    int64_t ld;
    int gauss, add_noise;
    PhiloxKey rng;
};
hipError_t launch_absent_visible(const AbsentVisibleArgs& a, hipStream_t s);

// rows of y [N][ld] whose row_count is 0 become NaN in columns < cols
hipError_t launch_absent_mark_rows(float* y, int64_t N, int64_t ld, int64_t cols, const int32_t* row_count, hipStream_t s);

// out[r] -= 1/2 sum_{i not observed} vbias[i]^2: what the zero-filled absent entries of a Gaussian row added to its free energy
hipError_t launch_absent_fe_fix(const uint32_t* observed, int64_t N, int64_t V, const float* vbias, float* out, hipStream_t s);

}  // namespace mdbn

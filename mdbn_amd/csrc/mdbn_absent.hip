// Absent visible units: CD on rows with missing entries (Salakhutdinov, Mnih & Hinton 2007).  Row r observes the set O_r of
// visible units; a unit outside O_r is absent from that row's RBM, and every row's RBM shares W, b, c.  On the device this is
// CD with a per-row mask: the row goes up zero-filled, comes down through absent_visible_kernel, which zeroes the absent
// entries again, and the unchanged statistics GEMM runs on the masked stacks.
//
//   absent_split_kernel     one workgroup per 256 columns of one row: NaN -> 0 (only NaN marks a missing entry; +-inf are
//                           values), the observed bits by one wave ballot per 64 columns (lane 0 stores the two words).  In
//                           place works: a thread reads its entry before it writes it.  Pad columns are neither read nor written.
//   absent_count_kernel     (only when row_count is wanted) one wave per row: popcount of its mask words.
//   absent_visible_kernel   the geometry and the Philox addressing of group_softmax_kernel without groups: one thread owns a
//                           4-row block of one column, 256 columns per workgroup.  Bernoulli: mean = sigmoidf_(x), sample =
//                           u < mean, cost = v0 softplus(-x) + (1 - v0) softplus(x) -- the arithmetic of act_quad_tg, bit for
//                           bit with every entry observed.  Gaussian: mean = x, sample = mean [+ N(0, 1) by Box-Muller from
//                           the draws `draw` and `draw | MDBN_NORMAL_BIT` with add_noise], cost = (sigmoid(x) - v0)^2.  An
//                           absent entry is 0 in mean, sample and tap and adds nothing to the cost.  One cost partial per
//                           workgroup (block_sum: fixed order), finished by finalize_stats_kernel.
//   absent_mark_rows_kernel rows nobody observed become rows of NaN.
//   absent_fe_fix_kernel    one workgroup per row: thread l adds vbias[i]^2 of the absent columns l, l + 256, ... in ascending
//                           order, block_sum adds the 256 partial sums in a fixed order; out[r] -= sum / 2.
//
// No atomics, every sum in a fixed order: two runs agree bit for bit.  The compiler's figures are in DESIGN.md 3.22.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_absent.h"
#include "mdbn_device.h"

namespace mdbn {
namespace {

__global__ __launch_bounds__(ABSENT_NT) void absent_split_kernel(AbsentSplitArgs a, int col_blocks, int words)
{
    const int bx = (int)blockIdx.x % col_blocks, r = (int)blockIdx.x / col_blocks;
    const int col = bx * ABSENT_NT + (int)threadIdx.x;
    bool seen = false;
    if (col < a.V) {
        const float x = a.x[(int64_t)r * a.ldx + col];
        seen = !(x != x);
        a.filled[(int64_t)r * a.ld_filled + col] = seen ? x : 0.0f;
    }
    const unsigned long long bits = __ballot(seen);
    if ((threadIdx.x & 63) == 0) {
        const int w = bx * (ABSENT_NT / 32) + 2 * ((int)threadIdx.x >> 6);
        uint32_t* dst = a.observed + (int64_t)r * words;
        if (w < words) dst[w] = (uint32_t)bits;
        if (w + 1 < words) dst[w + 1] = (uint32_t)(bits >> 32);
    }
}

__global__ __launch_bounds__(64) void absent_count_kernel(const uint32_t* observed, int words, int32_t* row_count)
{
    const uint32_t* src = observed + (int64_t)blockIdx.x * words;
    int n = 0;
    for (int w = (int)threadIdx.x; w < words; w += 64) n += __popc(src[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if (threadIdx.x == 0) row_count[blockIdx.x] = n;
}

__global__ __launch_bounds__(ABSENT_NT) void absent_visible_kernel(AbsentVisibleArgs a, int col_blocks, int words)
{
    __shared__ float red[4];
    const int bx = (int)blockIdx.x % col_blocks, by = (int)blockIdx.x / col_blocks;
    const int col = bx * ABSENT_NT + (int)threadIdx.x;
    const int r0 = 4 * by;
    float cost = 0.f;
    if (col < a.V) {
        const bool noisy = a.gauss != 0 && a.add_noise != 0;
        const bool need_u = (a.sample != nullptr || a.tap != nullptr) && (a.gauss == 0 || noisy);
        uint32_t wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
        if (need_u) {
            const uint64_t g0 = a.rng.row_offset + (uint64_t)r0;
            philox_rows4(a.rng, a.rng.draw, g0, (uint32_t)col, wa);
            if (noisy) philox_rows4(a.rng, a.rng.draw | MDBN_NORMAL_BIT, g0, (uint32_t)col, wb);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (r0 + j >= a.B) continue;
            const int64_t off = (int64_t)(r0 + j) * a.ld + col;
            const bool seen = (a.observed[(int64_t)(r0 + j) * words + (col >> 5)] >> (col & 31)) & 1u;
            const float x = a.pre[off];
            float m, sv;
            if (a.gauss) {
                m = x;
                sv = m;
                if (noisy) {
                    const float u1 = philox_u01(wa[j]), u2 = philox_u01(wb[j]);
                    sv = m + sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
                }
            } else {
                m = sigmoidf_(x);
                sv = philox_u01(wa[j]) < m ? 1.0f : 0.0f;
            }
            if (a.v0 && seen) {
                const float tg = a.v0[off];
                if (a.gauss) { const float d = sigmoidf_(x) - tg; cost += d * d; }
                else cost += tg * softplusf_(-x) + (1.0f - tg) * softplusf_(x);
            }
            if (!seen) { m = 0.f; sv = 0.f; }
            if (a.mean) a.mean[off] = m;
            if (a.sample) a.sample[off] = sv;
            if (a.tap) a.tap[off] = sv;
        }
    }
    if (a.cost_partials) {
        const float tot = block_sum(cost, red);
        if (threadIdx.x == 0) a.cost_partials[blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(ABSENT_NT) void absent_mark_rows_kernel(float* y, int64_t ld, int cols, const int32_t* row_count, int col_blocks)
{
    const int bx = (int)blockIdx.x % col_blocks, r = (int)blockIdx.x / col_blocks;
    const int col = bx * ABSENT_NT + (int)threadIdx.x;
    if (col < cols && row_count[r] == 0) y[(int64_t)r * ld + col] = __builtin_nanf("");
}

__global__ __launch_bounds__(ABSENT_NT) void absent_fe_fix_kernel(const uint32_t* observed, int V, int words, const float* vbias, float* out)
{
    __shared__ float red[4];
    const uint32_t* bits = observed + (int64_t)blockIdx.x * words;
    float acc = 0.f;
    for (int i = (int)threadIdx.x; i < V; i += ABSENT_NT) {
        const float b = vbias[i];
        if (!((bits[i >> 5] >> (i & 31)) & 1u)) acc = fmaf(b, b, acc);
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] -= 0.5f * tot;
}

}  // namespace

hipError_t launch_absent_split(const AbsentSplitArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.ldx < a.V || a.ld_filled < a.V || !a.x || !a.filled || !a.observed) return hipErrorInvalidValue;
    const int64_t blocks = absent_split_blocks(a.B, a.V);
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const int words = (int)absent_words(a.V);
    hipLaunchKernelGGL(absent_split_kernel, dim3((unsigned)blocks), dim3(ABSENT_NT), 0, s, a, (int)absent_col_blocks(a.V), words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.row_count) return e;
    hipLaunchKernelGGL(absent_count_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a.observed, words, a.row_count);
    return hipGetLastError();
}

hipError_t launch_absent_visible(const AbsentVisibleArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.ld < a.V || !a.pre || !a.observed || (a.v0 != nullptr) != (a.cost_partials != nullptr))
        return hipErrorInvalidValue;
    const int64_t blocks = absent_visible_blocks(a.B, a.V);
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(absent_visible_kernel, dim3((unsigned)blocks), dim3(ABSENT_NT), 0, s, a, (int)absent_col_blocks(a.V),
                       (int)absent_words(a.V));
    return hipGetLastError();
}

hipError_t launch_absent_mark_rows(float* y, int64_t N, int64_t ld, int64_t cols, const int32_t* row_count, hipStream_t s)
{
    if (N < 1 || cols < 1 || ld < cols || !y || !row_count) return hipErrorInvalidValue;
    const int64_t col_blocks = absent_col_blocks(cols), blocks = col_blocks * N;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(absent_mark_rows_kernel, dim3((unsigned)blocks), dim3(ABSENT_NT), 0, s, y, ld, (int)cols, row_count, (int)col_blocks);
    return hipGetLastError();
}

hipError_t launch_absent_fe_fix(const uint32_t* observed, int64_t N, int64_t V, const float* vbias, float* out, hipStream_t s)
{
    if (N < 1 || N > 0x7fffffff || V < 1 || !observed || !vbias || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(absent_fe_fix_kernel, dim3((unsigned)N), dim3(ABSENT_NT), 0, s, observed, (int)V, (int)absent_words(V), vbias, out);
    return hipGetLastError();
}

}  // namespace mdbn

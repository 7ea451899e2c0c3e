// Categorical visible units: grouped softmax sampling (Salakhutdinov, Mnih & Hinton 2007; the label block of the
// classification RBM of Larochelle & Bengio 2008).  A visible layer holds a contiguous span of adjacent groups -- group g is
// columns group_start[g] .. group_start[g + 1] - 1, exactly one of which is on -- between ordinary Bernoulli columns.
//
//   group_softmax_kernel   one thread owns a 4-row block of one unit (a group, or a Bernoulli column): the shape one Philox
//                          block serves.  Per row of a group, with m = max_c x_c:  e_c = __expf(x_c - m),  Z = sum_c e_c
//                          (ascending c, f32),  mean_c = e_c / Z (correctly rounded);  the category is the first c with
//                          u < C_c, C_c the running f32 sum of the stored means, and K - 1 when none qualifies (C_{K-1} may
//                          fall short of the largest uniform 1 - 2^-25); u is the uniform of the group's FIRST column.  A
//                          Bernoulli column is the arithmetic and addressing of the activation epilogue (act_quad_tg):
//                          mean = sigmoidf_(x), sample = u < mean.  Cost (optional): sum_c v0_c (log Z - (x_c - m)) for a group
//                          -- the cross-entropy from the log-sum-exp, finite where a probability underflows -- and the
//                          epilogue's v0 softplus(-x) + (1 - v0) softplus(x) for a Bernoulli column; one partial per workgroup
//                          (block_sum: fixed order), finished by finalize_stats_kernel.
//
//   center_rowdot_kernel,  the hidden-bias statistic of the centred gradient from the rows of the step's scratch (mdbn_groups.h,
//   center_hidden_kernel   CenterHiddenArgs): d_r = mu . (x_r - mu) by one workgroup per row of V2 (four accumulators per
//                          thread, block_sum), then s_h'_j by 64 hidden units x 4 row parts per workgroup, every sum in a
//                          fixed order.  No scratch; 16 bytes and 1 KB of LDS.
//
// No atomics, every sum in a fixed order: two runs agree bit for bit.  Pad columns V..ld-1 are neither read nor written.  A
// row of a group is walked three times (max, Z, means): the second and third read come from the cache, and K has no register
// cost.  gfx950, -O3: 24 VGPRs, 72 SGPRs, 0 bytes of scratch, 16 bytes of LDS (the four wave sums of block_sum).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_groups.h"
#include "mdbn_device.h"

namespace mdbn {
namespace {

__global__ __launch_bounds__(GROUPS_NT) void group_softmax_kernel(GroupSoftmaxArgs a, int unit_blocks)
{
    __shared__ float red[4];
    const int bx = (int)blockIdx.x % unit_blocks, by = (int)blockIdx.x / unit_blocks;
    const int unit = bx * GROUPS_NT + (int)threadIdx.x;
    const int r0 = 4 * by;
    float cost = 0.f;
    if (unit < a.units) {
        int c0, K = 0;                                   // first column; K = 0: a Bernoulli column
        if (unit < a.span_lo) {
            c0 = unit;
        } else if (unit < a.span_lo + a.n_groups) {
            const int g = unit - a.span_lo;
            // (the caller checked its host copy; the device copy is clamped to the span all the same)
            c0 = min(max(a.group_start[g], a.span_lo), a.span_hi - 1);
            K = min(min(max(a.group_start[g + 1], c0 + 1), a.span_hi) - c0, MDBN_GROUP_MAX);
        } else {
            c0 = a.span_hi + (unit - a.span_lo - a.n_groups);
        }
        const bool need_u = a.sample != nullptr || a.tap != nullptr;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (need_u) philox_rows4(a.rng, a.rng.draw, a.rng.row_offset + (uint64_t)r0, (uint32_t)c0, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (r0 + j >= a.B) continue;
            const int64_t off = (int64_t)(r0 + j) * a.ld + c0;
            const float u = philox_u01(w[j]);
            if (K == 0) {
                const float x = a.pre[off];
                const float m = sigmoidf_(x);
                const float sv = u < m ? 1.0f : 0.0f;
                if (a.v0) {
                    const float tg = a.v0[off];
                    cost += tg * softplusf_(-x) + (1.0f - tg) * softplusf_(x);
                }
                if (a.mean) a.mean[off] = m;
                if (a.sample) a.sample[off] = sv;
                if (a.tap) a.tap[off] = sv;
                continue;
            }
            const float* x = a.pre + off;
            float mx = x[0];
            for (int c = 1; c < K; ++c) mx = fmaxf(mx, x[c]);
            float Z = 0.f;
            for (int c = 0; c < K; ++c) Z += __expf(x[c] - mx);
            const float logZ = a.v0 ? __logf(Z) : 0.f;
            float cum = 0.f;
            bool found = false;
            for (int c = 0; c < K; ++c) {
                const float d = x[c] - mx;                  // (read before mean[off + c] is written: mean may be pre)
                const float m = __fdiv_rn(__expf(d), Z);
                cum += m;
                const bool hit = !found && (u < cum || c == K - 1);
                found = found || hit;
                if (a.v0) cost += a.v0[off + c] * (logZ - d);
                const float sv = hit ? 1.0f : 0.0f;
                if (a.mean) a.mean[off + c] = m;
                if (a.sample) a.sample[off + c] = sv;
                if (a.tap) a.tap[off + c] = sv;
            }
        }
    }
    if (a.cost_partials) {
        const float tot = block_sum(cost, red);
        if (threadIdx.x == 0) a.cost_partials[blockIdx.x] = tot;
    }
}

// one workgroup per row of V2 (then s_v, v_mean, mu): thread l adds the columns l, l + 256, ... in ascending order on four
// accumulators (column index / 256 mod 4: four loads in flight), combined as ((a0 + a1) + (a2 + a3)); block_sum adds the 256
// partial sums in a fixed order
__global__ __launch_bounds__(GROUPS_NT) void center_rowdot_kernel(CenterHiddenArgs a)
{
    __shared__ float red[4];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int extra = r - 2 * a.B;                       // 0: s_v . mu, 1: v_mean . mu, 2: mu . mu (the last two: sparsity)
    const float* x = extra < 0 ? a.V2 + (int64_t)r * a.ldv : extra == 0 ? a.stats + (int64_t)a.V * a.ldh + a.ldh
                   : extra == 1 ? a.v_mean : a.mu;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (x)
        for (int i0 = tid; i0 < a.V; i0 += 4 * GROUPS_NT) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * GROUPS_NT;
                if (i < a.V) {
                    const float m = a.mu[i];
                    acc[u] = fmaf(m, extra < 0 ? x[i] - m : x[i], acc[u]);
                }
            }
        }
    const float tot = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), red);
    if (tid == 0) a.d[r] = tot;
}

// 64 hidden units x 4 row parts per workgroup: part p adds the rows p, p + 4, ... of the 2B in ascending order (eight loads in
// flight), the four parts are added as ((p0 + p1) + (p2 + p3))
__global__ __launch_bounds__(GROUPS_NT) void center_hidden_kernel(CenterHiddenArgs a)
{
    __shared__ float part[4][64];
    const int c = (int)threadIdx.x & 63, p = (int)threadIdx.x >> 6;
    const int j = (int)blockIdx.x * 64 + c;
    float t = 0.f;
    if (j < a.H) {
#pragma unroll 8
        for (int r = p; r < 2 * a.B; r += 4) t = fmaf(a.d[r], a.P2[(int64_t)r * a.ldh + j], t);
    }
    part[p][c] = t;
    __syncthreads();
    if (p != 0 || j >= a.H) return;
    t = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
    const float s_h = a.stats[(int64_t)a.V * a.ldh + j];
    t -= a.d[2 * a.B] * a.lam[j];
    if (a.q) t += (a.w_scale * a.d[2 * a.B + 1] - a.b_scale * a.d[2 * a.B + 2]) * (a.target - a.q[j]);
    a.out[j] = s_h - a.rho * t;
}

}  // namespace

hipError_t launch_center_hidden(const CenterHiddenArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.H < 1 || a.ldv < a.V || a.ldh < a.H || !a.V2 || !a.P2 || !a.stats || !a.mu || !a.lam || !a.d || !a.out ||
        (a.q && a.w_scale != 0.f && !a.v_mean))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(center_rowdot_kernel, dim3((unsigned)(2 * a.B + (a.q ? 3 : 1))), dim3(GROUPS_NT), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(center_hidden_kernel, dim3((unsigned)((a.H + 63) / 64)), dim3(GROUPS_NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_softmax(const GroupSoftmaxArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.ld < a.V || !a.pre || a.n_groups < 0 || (a.n_groups > 0 && !a.group_start) ||
        a.span_lo < 0 || a.span_lo > a.span_hi || a.span_hi > a.V || (a.n_groups == 0) != (a.span_lo == a.span_hi) ||
        a.n_groups > a.span_hi - a.span_lo || a.units != group_units(a.V, a.span_lo, a.span_hi, a.n_groups) ||
        (a.v0 != nullptr) != (a.cost_partials != nullptr))
        return hipErrorInvalidValue;
    const int unit_blocks = (a.units + GROUPS_NT - 1) / GROUPS_NT;
    const int64_t blocks = group_softmax_blocks(a.B, a.units);
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_softmax_kernel, dim3((unsigned)blocks), dim3(GROUPS_NT), 0, s, a, unit_blocks);
    return hipGetLastError();
}

}  // namespace mdbn

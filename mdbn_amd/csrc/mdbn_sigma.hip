// Learned per-column variance of a Gaussian visible layer (Hinton's practical guide, section 13.2; Krizhevsky 2009; Cho et al.
// 2011), in the parametrisation p(x) = p_u(x exp(-s)) exp(-sum s): p_u is the unit-variance GRBM, s = log sigma.  The CD
// chain, the GEMMs and the statistics all run on u = x exp(-s), "the rows in units"; what is new is memory-bound:
//
//   sigma_scale_rows_kernel    dst[r, i] = src[idx[r], i] expf(sign s_i): the gather of a training step with the scaling in it
//                              (sign = -1), and the way back (sign = +1).  A thread owns four columns -- their factors are
//                              formed once, with expf --, walks the rows of its workgroup's row block four 16-byte loads in
//                              flight, and writes the pad columns V..ld_dst-1 of dst as zeros.  With s = 0 the factors are
//                              exactly 1.0f and the rows come out as gather_rows_kernel copies them.
//   sigma_update_kernel        q_i = sum_r U_ri (U_ri - M_ri) over the rows in ascending order (float32, compensated), a thread
//                              owning four columns; up to SIGMA_ONE_STAGE_ROWS rows one workgroup walks them all and applies
//                              the rule at once, above that the rows are split into slices of SIGMA_SLICE_ROWS whose partial
//                              sums go to the workspace and
//   sigma_finish_kernel        adds them in ascending slice order and applies the rule: g_i = q_i / n_rows - 1 (the -1 is the
//                              exact model expectation: no chain state enters), s_i = clamp(s_i + speed_i lr, lo, hi) with the
//                              OLD speed, speed_i = g_i + (speed_i - g_i) momentum -- the rule of the visible bias.
//
// No atomics, a fixed summation order: two runs agree bit for bit.  Pad columns of src, U and M are never read (a row's last
// 16-byte group is walked float by float when V is no multiple of 4).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "mdbn_sigma.h"
#include "mdbn_packed_walk.h"

namespace mdbn {
namespace {

__global__ __launch_bounds__(SIGMA_NT) void sigma_scale_rows_kernel(SigmaScaleArgs a)
{
    const int c = (int)blockIdx.x * SIGMA_NT + (int)threadIdx.x;          // the 16-byte group of columns 4c .. 4c + 3
    if (c >= (int)(a.ld_dst >> 2)) return;
    const int live = max(0, min(4, a.V - 4 * c));                        // (0: a group of pad columns, written as zeros)
    float4 f = load_live_scalar(a.log_sigma + 4 * c, live);
    f.x = expf(a.sign * f.x); f.y = expf(a.sign * f.y); f.z = expf(a.sign * f.z); f.w = expf(a.sign * f.w);
    const int r0 = (int)blockIdx.y * a.rows_per_block, r1 = min(a.B, r0 + a.rows_per_block);
    for (int r = r0; r < r1; r += 4) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r + u >= r1) continue;
            int64_t s = r + u;
            if (a.idx) s = a.idx64 ? reinterpret_cast<const int64_t*>(a.idx)[r + u] : (int64_t)reinterpret_cast<const int32_t*>(a.idx)[r + u];
            if (s < 0) s += a.n_src;                                      // numpy-style negative index
            s = s < 0 ? 0 : (s >= a.n_src ? a.n_src - 1 : s);             // never fault on a bad index
            x[u] = load_live(a.src + s * a.ld_src + 4 * c, live);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r + u >= r1) continue;
            // (the lanes that are not live hold 0 * expf(0): the pad columns come out as exact zeros)
            *reinterpret_cast<float4*>(a.dst + (int64_t)(r + u) * a.ld_dst + 4 * c) =
                make_float4(x[u].x * f.x, x[u].y * f.y, x[u].z * f.z, x[u].w * f.w);
        }
    }
}

struct Sum4 {                                                             // four compensated (Kahan) float32 sums side by side
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), comp = make_float4(0.f, 0.f, 0.f, 0.f);
    __device__ __forceinline__ static void add1(float& s, float& comp, float v)
    {
        const float y = v - comp, t = s + y;
        comp = (t - s) - y;
        s = t;
    }
    __device__ __forceinline__ void add(float4 v)
    {
        add1(s.x, comp.x, v.x); add1(s.y, comp.y, v.y); add1(s.z, comp.z, v.z); add1(s.w, comp.w, v.w);
    }
};

// sum over the rows r0 .. r1-1, ascending, of u (u - m) for the columns col .. col + live - 1
__device__ __forceinline__ float4 sigma_rows(const SigmaUpdateArgs& a, int col, int live, int r0, int r1)
{
    Sum4 acc;
    for (int r = r0; r < r1; r += 8) {                                    // eight rows of both matrices in flight
        float4 u[8], m[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (r + k >= r1) continue;
            u[k] = load_live(a.U + (int64_t)(r + k) * a.ldu + col, live);
            m[k] = load_live(a.M + (int64_t)(r + k) * a.ldm + col, live);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (r + k >= r1) continue;
            acc.add(make_float4(u[k].x * (u[k].x - m[k].x), u[k].y * (u[k].y - m[k].y), u[k].z * (u[k].z - m[k].z),
                                u[k].w * (u[k].w - m[k].w)));
        }
    }
    return acc.s;
}

// the rule on the live columns of one group, in place
__device__ __forceinline__ void sigma_finish(const SigmaUpdateArgs& a, int col, int live, float4 q)
{
    const float qs[4] = {q.x, q.y, q.z, q.w};
    const float inv = 1.0f / (float)a.n_rows;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= live) break;
        const float g = fmaf(qs[k], inv, -1.0f);
        const float speed = a.speed[col + k], s = a.log_sigma[col + k];
        a.log_sigma[col + k] = fminf(fmaxf(fmaf(speed, a.lr, s), a.lo), a.hi);
        a.speed[col + k] = fmaf(speed - g, a.momentum, g);
    }
}

__global__ __launch_bounds__(SIGMA_STAT_NT) void sigma_update_kernel(SigmaUpdateArgs a)
{
    const int col = 4 * ((int)blockIdx.x * SIGMA_STAT_NT + (int)threadIdx.x);
    if (col >= a.V) return;
    const int live = min(4, a.V - col);
    if (a.n_slices == 1) {
        sigma_finish(a, col, live, sigma_rows(a, col, live, 0, a.n_rows));
        return;
    }
    const int r0 = (int)blockIdx.y * SIGMA_SLICE_ROWS;
    const float4 q = sigma_rows(a, col, live, r0, min(a.n_rows, r0 + SIGMA_SLICE_ROWS));
    const int64_t ldp = ((int64_t)a.V + 3) & ~(int64_t)3;
    *reinterpret_cast<float4*>(a.partials + (int64_t)blockIdx.y * ldp + col) = q;
}

__global__ __launch_bounds__(SIGMA_STAT_NT) void sigma_finish_kernel(SigmaUpdateArgs a)
{
    const int col = 4 * ((int)blockIdx.x * SIGMA_STAT_NT + (int)threadIdx.x);
    if (col >= a.V) return;
    const int64_t ldp = ((int64_t)a.V + 3) & ~(int64_t)3;
    Sum4 acc;
    for (int s0 = 0; s0 < a.n_slices; s0 += 8) {                          // eight partials in flight, added in slice order
        float4 p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (s0 + k < a.n_slices) p[k] = *reinterpret_cast<const float4*>(a.partials + (int64_t)(s0 + k) * ldp + col);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (s0 + k < a.n_slices) acc.add(p[k]);
    }
    sigma_finish(a, col, min(4, a.V - col), acc.s);
}

}  // namespace

hipError_t launch_sigma_scale_rows(SigmaScaleArgs a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.n_src < 1 || a.ld_src < a.V || a.ld_dst < a.V || (a.ld_src & 3) || (a.ld_dst & 3) || !a.src || !a.dst ||
        !a.log_sigma || !(a.sign == 1.0f || a.sign == -1.0f))
        return hipErrorInvalidValue;
    const int64_t blocks_x = ((a.ld_dst >> 2) + SIGMA_NT - 1) / SIGMA_NT;
    int rpb = 4;                                  // rows of a workgroup: few while the grid is small, and gridDim.y has a limit
    while ((blocks_x * ((a.B + rpb - 1) / rpb) > 2048 && rpb < 32) || (a.B + rpb - 1) / rpb > 65535) rpb *= 2;
    a.rows_per_block = rpb;
    hipLaunchKernelGGL(sigma_scale_rows_kernel, dim3((unsigned)blocks_x, (unsigned)((a.B + rpb - 1) / rpb)), dim3(SIGMA_NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sigma_update(const SigmaUpdateArgs& a, hipStream_t s)
{
    if (a.n_rows < 1 || a.V < 1 || a.ldu < a.V || a.ldm < a.V || (a.ldu & 3) || (a.ldm & 3) || !a.U || !a.M || !a.log_sigma || !a.speed ||
        a.n_slices != sigma_slices(a.n_rows) || (a.n_slices > 1 && !a.partials) || a.n_slices > 65535)
        return hipErrorInvalidValue;
    const unsigned blocks_x = (unsigned)(((a.V + 3) / 4 + SIGMA_STAT_NT - 1) / SIGMA_STAT_NT);
    hipLaunchKernelGGL(sigma_update_kernel, dim3(blocks_x, (unsigned)a.n_slices), dim3(SIGMA_STAT_NT), 0, s, a);
    if (a.n_slices > 1) hipLaunchKernelGGL(sigma_finish_kernel, dim3(blocks_x), dim3(SIGMA_STAT_NT), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdbn

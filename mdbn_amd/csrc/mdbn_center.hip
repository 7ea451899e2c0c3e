// Centred CD training (Montavon & Mueller 2012; Cho et al. 2011; Melchior, Fischer & Wiskott 2016, Algorithm 1) for an RBM
// kept in its ordinary parameters: the centred gradient is a transform of the packed statistics [S | s_h | s_v | cost] of a
// CD step, applied between mdbn_cd_step and mdbn_apply_update.
//
//   center_offsets_kernel   column means of the data half of the step's scratch (v0 = rows 0..B-1 of V2, ph_mean = rows
//                           0..B-1 of P2) folded into the running offsets mu / lam.  One thread owns a column and adds its
//                           rows in ascending order (float32, compensated): a wave's loads of a row are contiguous.
//   center_stats_kernel     S'_ij = S_ij - mu_i s_h[j] - s_v[i] lam_j in place.  A workgroup owns a block of whole rows of S:
//                           it finishes s_v'[i] = s_v[i] - rho sum_j S'_ij lam_j of its rows and leaves its partial column
//                           sums sum_{i in block} mu_i S'_ij in the workspace.  S is read once and written once, 16 bytes
//                           per lane: the pass is memory-bound.
//   center_finish_kernel    s_h'[j] = s_h[j] - rho sum_blocks partial[block][j].  Every block of the pass above reads s_h,
//                           so it is written here only.
//
// No atomics, every sum in a fixed order: two runs agree bit for bit.  Pad columns H..ldh-1 of S and s_h and V..ldv-1 of s_v
// are neither read nor written (a row's last 16-byte group is walked float by float when H is no multiple of 4); the four
// cost floats are untouched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_center.h"
#include "mdbn_packed_walk.h"

namespace mdbn {
namespace {

constexpr int FIN_COLS = 64;                 // columns of a center_finish workgroup: one wave wide
constexpr int FIN_RUNS = 16;                 // its waves: each adds one contiguous run of the row blocks

__global__ __launch_bounds__(CENTER_OFF_NT) void center_offsets_kernel(CenterOffsetsArgs a, int blocks_v)
{
    const bool vis = (int)blockIdx.x < blocks_v;
    const int c = ((int)blockIdx.x - (vis ? 0 : blocks_v)) * CENTER_OFF_NT + (int)threadIdx.x;
    if (c >= (vis ? a.V : a.H)) return;
    const float m = column_mean((vis ? a.v0 : a.ph) + c, vis ? a.ldv : a.ldh, a.B);
    float* off = (vis ? a.mu : a.lam) + c;
    *off = a.nu == 1.0f ? m : fmaf(a.nu, m - *off, *off);
}

// CT threads side by side on a row (a multiple of the wave), CENTER_NT / CT rows side by side, NCH 16-byte groups of a row
// per thread (4 CT NCH >= H)
template <int CT, int NCH>
__global__ __launch_bounds__(CENTER_NT) void center_stats_kernel(CenterStatsArgs a)
{
    constexpr int RT = CENTER_NT / CT;
    constexpr int WR = CT / 64;              // waves that share a row
    static_assert(RT == 1 || NCH == 1, "several rows side by side only on rows one group per thread wide");
    __shared__ float rowpart[32][WR];        // a row's sum per wave
    __shared__ __attribute__((aligned(16))) float colpart[RT > 1 ? RT * CT * 4 : 4];
    const int tid = threadIdx.x, tx = tid % CT, ty = tid / CT, lane = tid & 63, wr = (tid >> 6) % WR;
    const int i0 = (int)blockIdx.x * a.rows;
    const int nrows = min(a.rows, a.V - i0);
    float* S = a.stats + (int64_t)i0 * a.ldh;
    const float* sh = a.stats + (int64_t)a.V * a.ldh;
    float* sv = a.stats + (int64_t)a.V * a.ldh + a.ldh + i0;
    const float* mu = a.mu + i0;

    int live[NCH];
    float4 shv[NCH], lmv[NCH], col[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int j = 4 * (tx + c * CT);
        live[c] = min(max(a.H - j, 0), 4);
        shv[c] = load_live_scalar(sh + j, live[c]);
        lmv[c] = load_live_scalar(a.lam + j, live[c]);
        col[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    for (int m = ty; m < nrows; m += 4 * RT) {           // four rows of this row lane in flight
        float mur[4], svr[4], rs[4];
        bool ok[4];                                      // (uniform over a wave: CT is a multiple of 64)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = m + u * RT;
            ok[u] = r < nrows;
            mur[u] = mu[min(r, nrows - 1)];
            svr[u] = sv[min(r, nrows - 1)];
            rs[u] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (live[c] == 0) continue;
            const int j = 4 * (tx + c * CT);
            float4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u]) x[u] = load_live(S + (int64_t)(m + u * RT) * a.ldh + j, live[c]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                float4 y;
                y.x = fmaf(-svr[u], lmv[c].x, fmaf(-mur[u], shv[c].x, x[u].x));
                y.y = fmaf(-svr[u], lmv[c].y, fmaf(-mur[u], shv[c].y, x[u].y));
                y.z = fmaf(-svr[u], lmv[c].z, fmaf(-mur[u], shv[c].z, x[u].z));
                y.w = fmaf(-svr[u], lmv[c].w, fmaf(-mur[u], shv[c].w, x[u].w));
                store_live(S + (int64_t)(m + u * RT) * a.ldh + j, live[c], y);
                rs[u] = fmaf(y.x, lmv[c].x, rs[u]);
                rs[u] = fmaf(y.y, lmv[c].y, rs[u]);
                rs[u] = fmaf(y.z, lmv[c].z, rs[u]);
                rs[u] = fmaf(y.w, lmv[c].w, rs[u]);
                col[c].x = fmaf(mur[u], y.x, col[c].x);
                col[c].y = fmaf(mur[u], y.y, col[c].y);
                col[c].z = fmaf(mur[u], y.z, col[c].z);
                col[c].w = fmaf(mur[u], y.w, col[c].w);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {                    // a row's sum: a fixed butterfly over the wave, the waves below
            float s = rs[u];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0 && ok[u]) rowpart[m + u * RT][wr] = s;
        }
    }
    if constexpr (RT > 1) *reinterpret_cast<float4*>(colpart + (ty * CT + tx) * 4) = col[0];
    __syncthreads();                                     // every read of s_v by this workgroup is behind us

    if (tid < nrows) {                                   // s_v' of the block's rows: the row's waves in ascending order
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WR; ++w) s += rowpart[tid][w];
        sv[tid] = fmaf(-a.rho, s, sv[tid]);
    }
    float* part = a.partial + (int64_t)blockIdx.x * a.ldp;
    if constexpr (RT > 1) {                              // the row lanes in ascending order
        if (ty == 0 && live[0] > 0) {
            float4 s = col[0];
#pragma unroll
            for (int t = 1; t < RT; ++t) {
                const float4 q = *reinterpret_cast<const float4*>(colpart + (t * CT + tx) * 4);
                s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
            }
            *reinterpret_cast<float4*>(part + 4 * tx) = s;
        }
    } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (live[c] > 0) *reinterpret_cast<float4*>(part + 4 * (tx + c * CT)) = col[c];
    }
}

// thread = (column j, run w of the row blocks): the runs are contiguous and ascending, each added in ascending order, then
// the runs in ascending order
__global__ __launch_bounds__(FIN_COLS * FIN_RUNS) void center_finish_kernel(CenterStatsArgs a)
{
    __shared__ float run[FIN_RUNS][FIN_COLS];
    const int tx = threadIdx.x & (FIN_COLS - 1), w = threadIdx.x / FIN_COLS;
    const int j = (int)blockIdx.x * FIN_COLS + tx;
    const int per = (a.blocks + FIN_RUNS - 1) / FIN_RUNS;
    const int b0 = min(w * per, a.blocks), b1 = min(b0 + per, a.blocks);
    float s = 0.f;
    if (j < a.H) {
        const float* p = a.partial + j;
        int b = b0;
        for (; b + 8 <= b1; b += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = p[(int64_t)(b + u) * a.ldp];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += t[u];
        }
        for (; b < b1; ++b) s += p[(int64_t)b * a.ldp];
    }
    run[w][tx] = s;
    __syncthreads();
    if (w == 0 && j < a.H) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < FIN_RUNS; ++q) t += run[q][tx];
        float* sh = a.stats + (int64_t)a.V * a.ldh;
        sh[j] = fmaf(-a.rho, t, sh[j]);
    }
}

}  // namespace

hipError_t launch_center_offsets(const CenterOffsetsArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.H < 1 || a.ldv < a.V || a.ldh < a.H || !(a.nu > 0.f && a.nu <= 1.f)) return hipErrorInvalidValue;
    const int blocks_v = (a.V + CENTER_OFF_NT - 1) / CENTER_OFF_NT, blocks_h = (a.H + CENTER_OFF_NT - 1) / CENTER_OFF_NT;
    hipLaunchKernelGGL(center_offsets_kernel, dim3((unsigned)(blocks_v + blocks_h)), dim3(CENTER_OFF_NT), 0, s, a, blocks_v);
    return hipGetLastError();
}

hipError_t launch_center_stats(const CenterStatsArgs& a, hipStream_t s)
{
    if (a.V < 1 || a.H < 1 || a.H > CENTER_MAX_H || a.ldh < a.H || (a.ldh & 3) || a.ldv < a.V || a.rows < 1 || a.rows > 32 ||
        a.blocks != (a.V + a.rows - 1) / a.rows || a.ldp != ((a.H + 3) & ~3))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.blocks), block(CENTER_NT);
    const int groups = (a.H + 3) / 4;
    if (groups <= 64) hipLaunchKernelGGL((center_stats_kernel<64, 1>), grid, block, 0, s, a);
    else if (groups <= 128) hipLaunchKernelGGL((center_stats_kernel<128, 1>), grid, block, 0, s, a);
    else if (groups <= 256) hipLaunchKernelGGL((center_stats_kernel<256, 1>), grid, block, 0, s, a);
    else if (groups <= 512) hipLaunchKernelGGL((center_stats_kernel<256, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((center_stats_kernel<256, CENTER_MAXCH>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(center_finish_kernel, dim3((unsigned)((a.H + FIN_COLS - 1) / FIN_COLS)), dim3(FIN_COLS * FIN_RUNS), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdbn

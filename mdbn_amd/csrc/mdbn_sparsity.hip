// Sparsity target for the hidden units (Lee, Ekanadham & Ng 2008; Nair & Hinton 2009; Hinton's practical guide, section
// 11): a penalty that drives every hidden unit's mean activation q_j towards a target p, as a second transform of the packed
// statistics [S | s_h | s_v | cost] of a CD step, applied between mdbn_cd_step and mdbn_apply_update (before the centring
// transform of mdbn_center.hip, when both are on).
//
//   sparsity_activity_kernel   column means of the data half of the step's scratch: of ph_mean (rows 0..B-1 of P2) folded
//                              into the running estimate q, and, when asked, of v0 (rows 0..B-1 of V2) written to v_mean.
//                              One thread owns a column and adds its rows in ascending order (float32, compensated).
//   sparsity_stats_kernel      S_ij += (w_scale v_mean[i]) (target - q_j) in place, by workgroups that own blocks of whole
//                              rows of S (the geometry of center_stats_kernel); the workgroup of row block 0 also does
//                              s_h[j] += b_scale (target - q_j).  Elementwise: S is read once and written once, 16 bytes
//                              per lane, and a thread walks the row in steps of the workgroup's width, so H has no limit.
//
// No atomics, no sum across threads: two runs agree bit for bit.  Pad columns H..ldh-1 of S and s_h are neither read nor
// written (a row's last 16-byte group is walked float by float when H is no multiple of 4); s_v and the four cost floats are
// untouched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_sparsity.h"
#include "mdbn_center.h"
#include "mdbn_packed_walk.h"

namespace mdbn {
namespace {

__global__ __launch_bounds__(COLUMN_MEAN_NT) void sparsity_activity_kernel(SparsityActivityArgs a, int blocks_h)
{
    const bool hid = (int)blockIdx.x < blocks_h;
    const int c = ((int)blockIdx.x - (hid ? 0 : blocks_h)) * COLUMN_MEAN_NT + (int)threadIdx.x;
    if (c >= (hid ? a.H : a.V)) return;
    const float m = column_mean((hid ? a.ph : a.v0) + c, hid ? a.ldh : a.ldv, a.B);
    if (hid) {
        float* q = a.q + c;
        *q = a.rate == 1.0f ? m : fmaf(a.rate, m - *q, *q);
    } else {
        a.v_mean[c] = m;
    }
}

// CT threads side by side on a row (a multiple of the wave), SPARSITY_NT / CT rows side by side; a thread takes the 16-byte
// groups tx, tx + CT, ... of its rows, four rows in flight
template <int CT>
__global__ __launch_bounds__(SPARSITY_NT) void sparsity_stats_kernel(SparsityStatsArgs a)
{
    constexpr int RT = SPARSITY_NT / CT;
    const int tid = threadIdx.x, tx = tid % CT, ty = tid / CT;
    const int i0 = (int)blockIdx.x * a.rows;
    const int nrows = a.w_scale != 0.f ? min(a.rows, a.V - i0) : 0;      // (w_scale = 0: one workgroup, the s_h half only)
    float* S = a.stats + (int64_t)i0 * a.ldh;
    float* sh = a.stats + (int64_t)a.V * a.ldh;
    const bool owner = blockIdx.x == 0 && ty == 0 && a.b_scale != 0.f;

    for (int j = 4 * tx; j < a.H; j += 4 * CT) {
        const int live = min(a.H - j, 4);
        const float4 q = load_live_scalar(a.q + j, live);
        const float4 t = make_float4(a.target - q.x, a.target - q.y, a.target - q.z, a.target - q.w);
        for (int m = ty; m < nrows; m += 4 * RT) {
            float ar[4];
            float4 x[4];
            bool ok[4];                                  // (uniform over a wave: CT is a multiple of 64)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = m + u * RT;
                ok[u] = r < nrows;
                ar[u] = a.w_scale * a.v_mean[i0 + min(r, nrows - 1)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u]) x[u] = load_live(S + (int64_t)(m + u * RT) * a.ldh + j, live);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                float4 y;
                y.x = fmaf(ar[u], t.x, x[u].x);
                y.y = fmaf(ar[u], t.y, x[u].y);
                y.z = fmaf(ar[u], t.z, x[u].z);
                y.w = fmaf(ar[u], t.w, x[u].w);
                store_live(S + (int64_t)(m + u * RT) * a.ldh + j, live, y);
            }
        }
        if (owner) {                                     // (nothing in this launch reads s_h)
            float4 s = load_live(sh + j, live);
            s.x = fmaf(a.b_scale, t.x, s.x);
            s.y = fmaf(a.b_scale, t.y, s.y);
            s.z = fmaf(a.b_scale, t.z, s.z);
            s.w = fmaf(a.b_scale, t.w, s.w);
            store_live(sh + j, live, s);
        }
    }
}

}  // namespace

hipError_t launch_sparsity_activity(const SparsityActivityArgs& a, hipStream_t s)
{
    const bool vis = a.v0 != nullptr;
    if (a.B < 1 || a.H < 1 || a.ldh < a.H || !a.ph || !a.q || vis != (a.v_mean != nullptr) || (vis && (a.V < 1 || a.ldv < a.V)) ||
        !(a.rate > 0.f && a.rate <= 1.f))
        return hipErrorInvalidValue;
    const int blocks_h = (a.H + COLUMN_MEAN_NT - 1) / COLUMN_MEAN_NT;
    const int blocks_v = vis ? (a.V + COLUMN_MEAN_NT - 1) / COLUMN_MEAN_NT : 0;
    hipLaunchKernelGGL(sparsity_activity_kernel, dim3((unsigned)(blocks_h + blocks_v)), dim3(COLUMN_MEAN_NT), 0, s, a, blocks_h);
    return hipGetLastError();
}

hipError_t launch_sparsity_stats(const SparsityStatsArgs& a, hipStream_t s)
{
    if (a.V < 1 || a.H < 1 || a.ldh < a.H || (a.ldh & 3) || !a.stats || !a.q || !(a.w_scale >= 0.f) || !(a.b_scale >= 0.f) ||
        (a.w_scale > 0.f && !a.v_mean) || a.rows != center_rows_per_block(a.V))
        return hipErrorInvalidValue;
    if (a.w_scale == 0.f && a.b_scale == 0.f) return hipSuccess;
    const dim3 grid((unsigned)(a.w_scale != 0.f ? center_blocks(a.V) : 1)), block(SPARSITY_NT);
    const int groups = (a.H + 3) / 4;
    if (groups <= 64) hipLaunchKernelGGL((sparsity_stats_kernel<64>), grid, block, 0, s, a);
    else if (groups <= 128) hipLaunchKernelGGL((sparsity_stats_kernel<128>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sparsity_stats_kernel<256>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace mdbn

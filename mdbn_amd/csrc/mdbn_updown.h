// Up-down fine-tuning of a DBN (Hinton, Osindero & Teh 2006; mdbn_updown.hip): the delta rules of the untied directed
// layers.  Arguments, geometry and launchers.
//
//   generative half   g = act(x_hi G^T + c),  S = (x_lo - g)^T x_hi,  s_v = sum_r (x_lo - g): updates G, its speed and c
//   recognition half  S = y_lo^T (y_hi - r),  s_h = sum_r (y_hi - r):                          updates W, its speed and b
//
// Both are CD statistics with chosen operands (V2 = [x_lo; g], P2 = [x_hi; -x_hi] and V2 = [y_lo; y_lo], P2 = [y_hi; -r]):
// updown_stack_kernel writes those stacked buffers, and the statistics and update launchers of the CD step do the rest on
// any shape.  For minibatches of <= 32 rows and ldh <= 512 updown_gen_kernel does the generative half in ONE pass over G.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"

namespace mdbn {

constexpr int UD_NT = 512;                  // threads of an updown_gen workgroup: 8 waves, one row of G each at a time
constexpr int UD_MAXB = 32;                 // minibatch rows of the one-pass kernel
constexpr int UD_MAX_LDH = 512;             // ... and its widest row of G (two 16-byte groups per lane)
constexpr int UD_MAX_RPW = 256;             // rows of G per workgroup
constexpr int UD_COST_NT = 256;             // threads of the cost-partial and cost-finish launches
constexpr int UD_COST_MAXG = 1024;          // workgroups of updown_cost_kernel

struct UpdownGeom {
    int Bq;                                 // minibatch rows rounded up to a multiple of 4
    int nch;                                // 16-byte groups of a row of G per lane (1 | 2)
    int rpw, G;                             // rows of G per workgroup (contiguous ranges), workgroups
    int lds;                                // dynamic LDS (bytes): x_hi [Bq][ldh] | x_lo^T [rpw][Bq] | a cost per wave
};

// Does the one-pass generative kernel serve this shape?  n <= 32, ldh <= 512: the regime of the thin-batch CD step.
__host__ __device__ inline bool updown_geom(int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int num_cu, UpdownGeom& t)
{
    if (n < 1 || n > UD_MAXB || V < 1 || H < 1 || ldh < H || ldv < V || ldh > UD_MAX_LDH || (ldh & 3) || (ldv & 3) ||
        V > (int64_t)1 << 24)
        return false;
    t.Bq = (int)((n + 3) & ~int64_t(3));
    t.nch = ldh <= 256 ? 1 : 2;
    const int cus = num_cu > 0 ? num_cu : 1;
    int64_t rpw = (V + cus - 1) / cus;                     // one workgroup of 8 waves per CU, every wave a round ahead with its loads
    if (rpw < 4) rpw = 4;
    if (rpw > UD_MAX_RPW) rpw = UD_MAX_RPW;
    t.rpw = (int)rpw;
    t.G = (int)((V + rpw - 1) / rpw);
    t.lds = (t.Bq * (int)ldh + t.rpw * t.Bq + UD_NT / 64) * 4;
    return true;
}

struct UpdownGenArgs {
    int n, Bq, V, H;
    int64_t ldv, ldh;
    int rpw, G;
    const float* x_lo; const float* x_hi;   // [n][ldv], [n][ldh]
    int gauss;                              // 0: sigmoid prediction, cross-entropy cost; 1: linear prediction, half squared error
    UpdEpi upd;                             // G, its speed, W0 (nullable), lr, l1, l2, wc, mu, inv_bs, planes of the new G or NULL
    float* vb; float* vbs;                  // [V] generative bias and its speed
    float inv_rows;
    float* cost_partials;                   // [G]: one per workgroup
};

// The one-pass generative kernel of a layer with softmax groups (updown_gen_grouped_kernel): the geometry of updown_geom, its
// workgroups' ranges moved onto group boundaries.  A range grows by at most UD_GROUP_SLACK rows (a group has at most
// MDBN_GROUP_MAX = 64 columns), and next to x_lo^T the workgroup holds the pre-activations (then the errors) of its rows:
// dynamic LDS x_hi [Bq][ldh] | x_lo^T [rpw + 63][Bq] | pre / err [rpw + 63][Bq] | two costs per wave.  At Bq = 32, ldh = 512,
// rpw = 256 that is 147 264 bytes of the CU's 160 KB: the row cap of the plain kernel stands.
constexpr int UD_GROUP_SLACK = 63;
constexpr int UD_GROUPED_MAX_LDS = (UD_MAXB * UD_MAX_LDH + 2 * (UD_MAX_RPW + UD_GROUP_SLACK) * UD_MAXB + 2 * (UD_NT / 64)) * 4;
static_assert(UD_GROUPED_MAX_LDS <= 160 * 1024, "updown_gen_grouped_kernel: the LDS of the widest shape must fit a CU");

__host__ __device__ inline bool updown_geom_grouped(int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int num_cu, UpdownGeom& t)
{
    if (!updown_geom(n, V, H, ldv, ldh, num_cu, t)) return false;
    t.lds = (t.Bq * (int)ldh + 2 * (t.rpw + UD_GROUP_SLACK) * t.Bq + 2 * (UD_NT / 64)) * 4;
    return true;
}

struct UpdownGenGroupedArgs {
    UpdownGenArgs g;                        // gauss = 0
    const int32_t* group_start;             // [n_groups + 1], device; clamped to the span below
    int n_groups, span_lo, span_hi;         // the span the caller's host copy gives
};

// V2 = [lo; second], P2 = [hi; -neg]: the stacked operands of mdbn_cd_stats.  Pad columns are written as zeros.
struct UpdownStackArgs {
    int n, V, H;
    int64_t ldv, ldh;
    const float* lo; const float* second;   // [n][ldv] each
    const float* hi; const float* neg;      // [n][ldh] each
    float* V2; float* P2;                   // [2n][ldv], [2n][ldh]
};

// cost partials of the composed generative half: cross-entropy of x against sigmoid(pre), or half squared error against
// the linear mean
struct UpdownCostArgs {
    int n, V, gauss, G;
    int64_t ldv;
    const float* x; const float* pre;       // [n][ldv] each (gauss: pre is the mean)
    float* cost_partials;                   // [G]
};

hipError_t launch_updown_gen(const UpdownGenArgs& a, const UpdownGeom& t, hipStream_t s);
hipError_t launch_updown_gen_grouped(const UpdownGenGroupedArgs& a, const UpdownGeom& t, hipStream_t s);
hipError_t launch_updown_stack(const UpdownStackArgs& a, hipStream_t s);
hipError_t launch_updown_cost(const UpdownCostArgs& a, hipStream_t s);
// cost_out[0] = (sum of the partials, ascending, in float64) * scale
hipError_t launch_updown_cost_finish(const float* partials, int n, float scale, float* cost_out, hipStream_t s);

}  // namespace mdbn

// Up-down fine-tuning of a DBN (Hinton, Osindero & Teh 2006, contrastive wake-sleep): the delta rules of the untied
// directed layers, between the wake / sleep passes (propup / propdown) and the engine's update rule (rbm.py:347-365).
//
//   updown_gen_kernel     the generative half in ONE pass over G for minibatches of <= 32 rows on rows of <= 512 floats.
//                         A workgroup owns a contiguous range of rows of G (visible units) and holds x_hi [Bq][ldh] and its
//                         columns of x_lo in LDS.  A wave takes one row at a time: its lanes hold the row of G and of the
//                         speed in registers (16 bytes per lane and group, the next row requested a round ahead), form the Bq partial dot
//                         products with x_hi by fmaf chains (float32 operands: no bf16 anywhere), reduce them over the wave
//                         with a fixed halving exchange (32 values in 32 shuffles), add the bias, apply the activation, take
//                         the error against x_lo, and with the errors as wave-uniform scalars form the row of
//                         S = (x_lo - g)^T x_hi in registers and hand it to the update rule at once: G and its speed are
//                         read once and written once, S is never stored.  The row's bias sum, its bias update and its cost
//                         term come from the same errors.  One cost partial per workgroup.
//   updown_gen_grouped_kernel   updown_gen_kernel for a layer whose visible units hold a span of softmax groups (the input
//                         layer of a network with visible_groups): the workgroups' row ranges moved onto group boundaries, the
//                         pre-activations of the span rows through LDS, the softmax there, a second walk over the span rows.
//                         updown_gen_kernel itself is left as it was: the plain call runs the code it ran.
//   updown_stack_kernel   V2 = [lo; second], P2 = [hi; -neg]: the stacked operands of mdbn_cd_stats (composed path, and the
//                         recognition half's one-pass update through thin_update_kernel).
//   updown_cost_kernel    cost partials of the composed generative half.
//   updown_cost_finish_kernel   the partials summed in ascending order (float64), times the scale.
//
// No atomics, every sum in a fixed order: two runs agree bit for bit.  updown_gen_kernel neither reads nor writes the pad
// columns H..ldh-1 of G, of the speed and of x_hi (a row's last 16-byte group is walked float by float when H is no multiple
// of 4); pad rows of the minibatch contribute exact zeros.  One instantiation per minibatch rows rounded up to 4 (Bq): the
// products run over Bq rows, the wave reduction over the next power of two.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_updown.h"
#include "mdbn_device.h"
#include "mdbn_packed_walk.h"

namespace mdbn {
namespace {

extern __shared__ __align__(16) float ud_smem[];

__device__ __forceinline__ float4 ud_lds4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Sums over the wave of N values per lane: every stage halves the values a lane carries while it exchanges the other half
// with the lane OFF away, so 32 sums cost 16 + 8 + 4 + 2 + 1 + 1 shuffles.  Afterwards every lane of the group
// lane >> (6 - log2 N) holds the sum of value number (lane >> (6 - log2 N)).  The order of the additions is fixed.
template <int N, int OFF>
struct RowReduce {
    static __device__ __forceinline__ float run(const float* v, int lane)
    {
        const bool up = (lane & OFF) != 0;
        float w[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) {
            const float send = up ? v[k] : v[k + N / 2];
            const float keep = up ? v[k + N / 2] : v[k];
            w[k] = keep + __shfl_xor(send, OFF, 64);
        }
        return RowReduce<N / 2, OFF / 2>::run(w, lane);
    }
};
template <int OFF>
struct RowReduce<1, OFF> {
    static __device__ __forceinline__ float run(const float* v, int)
    {
        float s = v[0];
#pragma unroll
        for (int off = OFF; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        return s;
    }
};

// BQ: the minibatch rows rounded up to 4 (the rows every product runs over); RB: the next power of two, the width of the
// wave reduction (its entries BQ..RB-1 are constant zeros)
template <int BQ, int NCH>
__global__ __launch_bounds__(UD_NT) void updown_gen_kernel(UpdownGenArgs a)
{
    constexpr int NW = UD_NT / 64;
    constexpr int RB = BQ <= 4 ? 4 : BQ <= 8 ? 8 : BQ <= 16 ? 16 : 32;
    constexpr int LB = RB == 4 ? 2 : RB == 8 ? 3 : RB == 16 ? 4 : 5;
    constexpr int GS = 6 - LB;                               // log2 of the lanes that end up with the same row's sum
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x;
    const int r0 = g * a.rpw, nrows = min(a.rpw, a.V - r0);
    const int ldh = (int)a.ldh;
    float* xh = ud_smem;                                     // [BQ][ldh]: pad rows and pad columns exact zeros
    float* xl = xh + BQ * ldh;                               // [rpw][BQ]: x_lo[., r0 + i]
    float* wcost = xl + a.rpw * BQ;                          // [NW]

    const int q4 = ldh >> 2;
    for (int e = tid; e < BQ * q4; e += UD_NT) {
        const int b = e / q4, j = 4 * (e - b * q4);
        const int lv = min(max(a.H - j, 0), 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < a.n && lv > 0) v = load_live(a.x_hi + (int64_t)b * a.ldh + j, lv);
        *reinterpret_cast<float4*>(xh + b * ldh + j) = v;
    }
    for (int e = tid; e < BQ * a.rpw; e += UD_NT) {
        const int b = e / a.rpw, i = e - b * a.rpw;          // (consecutive threads: consecutive columns of one row of x_lo)
        float v = 0.f;
        if (b < a.n && i < nrows) v = a.x_lo[(int64_t)b * a.ldv + r0 + i];
        xl[i * BQ + b] = v;
    }
    __syncthreads();

    const UpdEpi& u = a.upd;
    const float two_lr_l1 = upd_two_lr_l1(u.lr, u.l1);
    const float decay = upd_decay(u.lr, u.l2);
    int jj[NCH], live[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int j = 4 * lane + 256 * c;
        live[c] = min(max(a.H - j, 0), 4);
        jj[c] = live[c] > 0 ? j : 0;                         // (a dead group reads LDS at a valid place and multiplies it by zeros)
    }
    const int b_own = lane >> GS;
    const bool owner = (lane & ((1 << GS) - 1)) == 0 && b_own < a.n;
    float cost = 0.f;

    // A wave takes the rows wave, wave + NW, ... of the block; the row after the current one is requested before the current
    // one is worked on, so its loads are in flight while this row is reduced and updated (a wave owns its rows: nothing it
    // requests ahead is written by another)
    auto fetch = [&](int i, float4 (&fw)[NCH], float4 (&fs)[NCH]) {
        const int64_t off = (int64_t)(r0 + i) * a.ldh;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            fw[c] = fs[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[c] > 0) {
                fw[c] = load_live(u.W + off + jj[c], live[c]);
                fs[c] = load_live(u.Ws + off + jj[c], live[c]);
            }
        }
    };
    float4 w[NCH], sp[NCH];
    if (wave < nrows) fetch(wave, w, sp);
    for (int ii = wave; ii < nrows; ii += NW) {
        float4 nw[NCH], nsp[NCH];
        const bool more = ii + NW < nrows;                   // (uniform over the wave)
        if (more) fetch(ii + NW, nw, nsp);
        const int row = r0 + ii;
        // the prediction's product: Bq dot products of this row of G with the rows of x_hi
        float acc[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) acc[b] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                const float4 x = ud_lds4(xh + b * ldh + jj[c]);
                acc[b] = fmaf(w[c].x, x.x, acc[b]);
                acc[b] = fmaf(w[c].y, x.y, acc[b]);
                acc[b] = fmaf(w[c].z, x.z, acc[b]);
                acc[b] = fmaf(w[c].w, x.w, acc[b]);
                if ((b & 7) == 7) __asm__ volatile("" ::: "memory");      // (at most 8 LDS reads ahead: registers)
            }
        }
        const float dot = RowReduce<RB, 32>::run(acc, lane);
        // (x_hi is read from LDS again for the row of S: kept in registers across the reduction, its Bq 16-byte groups per
        //  column group would cost the occupancy that hides the row loads)
        __asm__ volatile("" ::: "memory");
        const float vb0 = a.vb[row], vs0 = a.vbs[row];
        const float x = xl[ii * BQ + min(b_own, BQ - 1)];
        const float p = dot + vb0;
        const float gv = a.gauss ? p : sigmoidf_(p);
        const float err = b_own < a.n ? x - gv : 0.f;
        float term = 0.f;
        if (owner) term = a.gauss ? 0.5f * err * err : x * softplusf_(-p) + (1.0f - x) * softplusf_(p);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off, 64);
        cost += term;
        // the errors of the minibatch rows as wave-uniform scalars; their sum in ascending order
        float eb[BQ];
        float sv = 0.f;
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            eb[b] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(err), b << GS));
            sv += eb[b];
        }
        const int64_t off = (int64_t)row * a.ldh;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (live[c] == 0) continue;
            float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                const float4 xv = ud_lds4(xh + b * ldh + jj[c]);
                st.x = fmaf(eb[b], xv.x, st.x);
                st.y = fmaf(eb[b], xv.y, st.y);
                st.z = fmaf(eb[b], xv.z, st.z);
                st.w = fmaf(eb[b], xv.w, st.w);
                if ((b & 7) == 7) __asm__ volatile("" ::: "memory");
            }
            // (a frozen weight-cost snapshot is a rare fifth stream: read where it is used)
            const float4 wc0 = u.W0 ? load_live(u.W0 + off + jj[c], live[c]) : w[c];
            float4 wn, sn;
            update_rule4(w[c], sp[c], st, wc0, u.inv_bs, u.wc, decay, u.l1, two_lr_l1, u.mu, u.lr, wn, sn);
            store_live(u.W + off + jj[c], live[c], wn);
            store_live(u.Ws + off + jj[c], live[c], sn);
            if (u.Wp) {                                      // bf16 planes of G, where a caller keeps some: the split of the new row
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= live[c]) break;
                    unsigned short q1, q2, q3;
                    split3(comp(wn, k), q1, q2, q3);
                    const int64_t o = off + jj[c] + k;
                    u.Wp[o] = q1; u.Wp[u.wp_stride + o] = q2; u.Wp[2 * u.wp_stride + o] = q3;
                }
            }
        }
        if (lane == 0) {                                     // the bias of this visible unit (rbm.py:356-365; the old speed moves it)
            a.vbs[row] = upd_speed(upd_scale(sv, a.inv_rows), vs0, u.mu);
            a.vb[row] = upd_param(vb0, 1.0f, vs0, u.lr);
        }
        if (more) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) { w[c] = nw[c]; sp[c] = nsp[c]; }
        }
    }
    if (lane == 0) wcost[wave] = cost;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) t += wcost[k];
        a.cost_partials[g] = t;
    }
}

// The device table clamped to the span the host copy gave (a stale device copy gives wrong groups, never an access outside)
__device__ __forceinline__ int ud_bound(const UpdownGenGroupedArgs& q, int k)
{
    return min(max(q.group_start[k], q.span_lo), q.span_hi);
}

// the smallest k in [0, n_groups] whose boundary is >= v (n_groups when none is)
__device__ __forceinline__ int ud_lower_bound(const UpdownGenGroupedArgs& q, int v)
{
    int lo = 0, hi = q.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ud_bound(q, mid) < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A nominal range edge moved off the inside of a group: forward to the end of the group that holds it, so that a group
// belongs to the workgroup whose nominal range holds its first row.  At most UD_GROUP_SLACK rows, whatever the table says.
__device__ __forceinline__ int ud_edge(const UpdownGenGroupedArgs& q, int e)
{
    if (e <= q.span_lo || e >= q.span_hi) return e;
    const int b = ud_bound(q, ud_lower_bound(q, e));
    return min(max(b, e), min(e + UD_GROUP_SLACK, q.span_hi));
}

// updown_gen_kernel for a layer whose rows of G (visible units) hold a span of softmax groups: g = softmax inside every
// group, sigmoid on the other rows.  A group's softmax needs the pre-activations of all its rows, which different waves form:
//   ranges       every workgroup moves the two edges of its nominal range [g rpw, (g + 1) rpw) forward off the inside of a
//                group (ud_edge); a range grows by at most 63 rows and may become empty (only a cost partial of 0 is written)
//   first walk   rows as in updown_gen_kernel.  A row outside the span is finished at once, by that kernel's arithmetic; a
//                row inside the span leaves pre[b] = dot + vbias for the Bq minibatch rows in LDS (its speed is not loaded)
//   softmax      one thread per (group, minibatch row), the arithmetic of group_softmax_kernel: m = max, e_c = __expf(x_c - m),
//                Z in ascending c, mean_c = e_c / Z; every entry becomes err = x - mean (0 in a pad minibatch row); the cost
//                term m + log Z - sum_c x_c pre_c is linear in x: the 1 is never looked for
//   second walk  the span rows again: the row of G once more (from cache), the row of the speed for the first time, the Bq
//                errors from LDS as broadcasts, the row of S, the rule, the planes, the bias
// Four HBM streams as before; no atomics, every sum in a fixed order; pad columns H..ldh-1 neither read nor written.
template <int BQ, int NCH>
__global__ __launch_bounds__(UD_NT) void updown_gen_grouped_kernel(UpdownGenGroupedArgs q)
{
    constexpr int NW = UD_NT / 64;
    constexpr int RB = BQ <= 4 ? 4 : BQ <= 8 ? 8 : BQ <= 16 ? 16 : 32;
    constexpr int LB = RB == 4 ? 2 : RB == 8 ? 3 : RB == 16 ? 4 : 5;
    constexpr int GS = 6 - LB;
    const UpdownGenArgs& a = q.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x;
    const int cap = a.rpw + UD_GROUP_SLACK;
    const int r0 = ud_edge(q, min(g * a.rpw, a.V));
    const int nrows = min(max(ud_edge(q, min((g + 1) * a.rpw, a.V)) - r0, 0), cap);      // (uniform over the workgroup)
    if (nrows == 0) {
        if (tid == 0) a.cost_partials[g] = 0.f;
        return;
    }
    // the span rows of this range [s0, s1) (relative to r0) and its groups [k0, k1)
    const int s0 = min(max(q.span_lo - r0, 0), nrows), s1 = max(min(q.span_hi - r0, nrows), s0);
    const int k0 = s1 > s0 ? ud_lower_bound(q, r0 + s0) : 0;
    const int k1 = s1 > s0 ? max(ud_lower_bound(q, r0 + s1), k0) : 0;
    const int ldh = (int)a.ldh;
    float* xh = ud_smem;                                     // [BQ][ldh]: pad rows and pad columns exact zeros
    float* xl = xh + BQ * ldh;                               // [cap][BQ]: x_lo[., r0 + i]
    float* pe = xl + cap * BQ;                               // [cap][BQ]: span rows: pre-activations, then errors
    float* wcost = pe + cap * BQ;                            // [NW] the walks' cost, [NW] the groups'

    const int q4 = ldh >> 2;
    for (int e = tid; e < BQ * q4; e += UD_NT) {
        const int b = e / q4, j = 4 * (e - b * q4);
        const int lv = min(max(a.H - j, 0), 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < a.n && lv > 0) v = load_live(a.x_hi + (int64_t)b * a.ldh + j, lv);
        *reinterpret_cast<float4*>(xh + b * ldh + j) = v;
    }
    for (int e = tid; e < BQ * nrows; e += UD_NT) {
        const int b = e / nrows, i = e - b * nrows;
        float v = 0.f;
        if (b < a.n) v = a.x_lo[(int64_t)b * a.ldv + r0 + i];
        xl[i * BQ + b] = v;
    }
    __syncthreads();

    const UpdEpi& u = a.upd;
    const float two_lr_l1 = upd_two_lr_l1(u.lr, u.l1);
    const float decay = upd_decay(u.lr, u.l2);
    int jj[NCH], live[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int j = 4 * lane + 256 * c;
        live[c] = min(max(a.H - j, 0), 4);
        jj[c] = live[c] > 0 ? j : 0;
    }
    const int b_own = lane >> GS;
    const bool owner = (lane & ((1 << GS) - 1)) == 0 && b_own < a.n;
    float cost = 0.f;

    // (speed: the row of the speed as well; a span row's speed waits for the second walk)
    auto fetch = [&](int i, bool speed, float4 (&fw)[NCH], float4 (&fs)[NCH]) {
        const int64_t off = (int64_t)(r0 + i) * a.ldh;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            fw[c] = fs[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[c] > 0) {
                fw[c] = load_live(u.W + off + jj[c], live[c]);
                if (speed) fs[c] = load_live(u.Ws + off + jj[c], live[c]);
            }
        }
    };
    // the row of S from the errors eb, the rule, the planes and the bias of row ii: updown_gen_kernel's statements
    auto finish = [&](int ii, const float (&eb)[BQ], float sv, float vb0, float vs0, const float4 (&w)[NCH], const float4 (&sp)[NCH]) {
        const int row = r0 + ii;
        const int64_t off = (int64_t)row * a.ldh;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (live[c] == 0) continue;
            float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                const float4 xv = ud_lds4(xh + b * ldh + jj[c]);
                st.x = fmaf(eb[b], xv.x, st.x);
                st.y = fmaf(eb[b], xv.y, st.y);
                st.z = fmaf(eb[b], xv.z, st.z);
                st.w = fmaf(eb[b], xv.w, st.w);
                if ((b & 7) == 7) __asm__ volatile("" ::: "memory");
            }
            const float4 wc0 = u.W0 ? load_live(u.W0 + off + jj[c], live[c]) : w[c];
            float4 wn, sn;
            update_rule4(w[c], sp[c], st, wc0, u.inv_bs, u.wc, decay, u.l1, two_lr_l1, u.mu, u.lr, wn, sn);
            store_live(u.W + off + jj[c], live[c], wn);
            store_live(u.Ws + off + jj[c], live[c], sn);
            if (u.Wp) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= live[c]) break;
                    unsigned short q1, q2, q3;
                    split3(comp(wn, k), q1, q2, q3);
                    const int64_t o = off + jj[c] + k;
                    u.Wp[o] = q1; u.Wp[u.wp_stride + o] = q2; u.Wp[2 * u.wp_stride + o] = q3;
                }
            }
        }
        if (lane == 0) {
            a.vbs[row] = upd_speed(upd_scale(sv, a.inv_rows), vs0, u.mu);
            a.vb[row] = upd_param(vb0, 1.0f, vs0, u.lr);
        }
    };
    auto in_span = [&](int i) { return i >= s0 && i < s1; };

    // ---- first walk
    {
        float4 w[NCH], sp[NCH];
        if (wave < nrows) fetch(wave, !in_span(wave), w, sp);
        for (int ii = wave; ii < nrows; ii += NW) {
            float4 nw[NCH], nsp[NCH];
            const bool more = ii + NW < nrows;
            if (more) fetch(ii + NW, !in_span(ii + NW), nw, nsp);
            const int row = r0 + ii;
            float acc[RB];
#pragma unroll
            for (int b = 0; b < RB; ++b) acc[b] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
#pragma unroll
                for (int b = 0; b < BQ; ++b) {
                    const float4 x = ud_lds4(xh + b * ldh + jj[c]);
                    acc[b] = fmaf(w[c].x, x.x, acc[b]);
                    acc[b] = fmaf(w[c].y, x.y, acc[b]);
                    acc[b] = fmaf(w[c].z, x.z, acc[b]);
                    acc[b] = fmaf(w[c].w, x.w, acc[b]);
                    if ((b & 7) == 7) __asm__ volatile("" ::: "memory");
                }
            }
            const float dot = RowReduce<RB, 32>::run(acc, lane);
            __asm__ volatile("" ::: "memory");
            const float vb0 = a.vb[row];
            const float p = dot + vb0;
            if (in_span(ii)) {                               // (uniform over the wave)
                if ((lane & ((1 << GS) - 1)) == 0 && b_own < BQ) pe[ii * BQ + b_own] = p;
            } else {
                const float vs0 = a.vbs[row];
                const float x = xl[ii * BQ + min(b_own, BQ - 1)];
                const float gv = sigmoidf_(p);
                const float err = b_own < a.n ? x - gv : 0.f;
                float term = 0.f;
                if (owner) term = x * softplusf_(-p) + (1.0f - x) * softplusf_(p);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off, 64);
                cost += term;
                float eb[BQ];
                float sv = 0.f;
#pragma unroll
                for (int b = 0; b < BQ; ++b) {
                    eb[b] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(err), b << GS));
                    sv += eb[b];
                }
                finish(ii, eb, sv, vb0, vs0, w, sp);
            }
            if (more) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) { w[c] = nw[c]; sp[c] = nsp[c]; }
            }
        }
    }
    float gcost = 0.f;
    if (s1 > s0) {                                           // (uniform over the workgroup)
        __syncthreads();
        // ---- softmax: item e = (group k0 + e / BQ, minibatch row e % BQ), a thread's items in ascending order
        const int items = (k1 - k0) * BQ;
        for (int e = tid; e < items; e += UD_NT) {
            const int k = k0 + e / BQ, b = e % BQ;
            const int c0 = min(max(ud_bound(q, k) - r0, s0), s1);
            const int K = min(min(max(ud_bound(q, k + 1) - r0, c0), s1) - c0, MDBN_GROUP_MAX);
            float* x = pe + c0 * BQ + b;
            const float* t = xl + c0 * BQ + b;
            if (b >= a.n || K < 1) {
                for (int c = 0; c < K; ++c) x[c * BQ] = 0.f;
                continue;
            }
            float mx = x[0];
            for (int c = 1; c < K; ++c) mx = fmaxf(mx, x[c * BQ]);
            float Z = 0.f;
            for (int c = 0; c < K; ++c) Z += __expf(x[c * BQ] - mx);
            float lin = 0.f;
            for (int c = 0; c < K; ++c) {
                const float pr = x[c * BQ], tg = t[c * BQ];
                lin = fmaf(tg, pr, lin);
                x[c * BQ] = tg - __fdiv_rn(__expf(pr - mx), Z);
            }
            gcost += (mx + __logf(Z)) - lin;
        }
        __syncthreads();
        // ---- second walk: the span rows
        float4 w[NCH], sp[NCH];
        if (s0 + wave < s1) fetch(s0 + wave, true, w, sp);
        for (int ii = s0 + wave; ii < s1; ii += NW) {
            float4 nw[NCH], nsp[NCH];
            const bool more = ii + NW < s1;
            if (more) fetch(ii + NW, true, nw, nsp);
            const int row = r0 + ii;
            const float vb0 = a.vb[row], vs0 = a.vbs[row];
            float eb[BQ];
            float sv = 0.f;
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                eb[b] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pe[ii * BQ + b])));     // (wave-uniform)
                sv += eb[b];
            }
            finish(ii, eb, sv, vb0, vs0, w, sp);
            if (more) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) { w[c] = nw[c]; sp[c] = nsp[c]; }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) gcost += __shfl_xor(gcost, off, 64);
    if (lane == 0) { wcost[wave] = cost; wcost[NW + wave] = gcost; }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * NW; ++k) t += wcost[k];
        a.cost_partials[g] = t;
    }
}

__global__ __launch_bounds__(256) void updown_stack_kernel(UpdownStackArgs a)
{
    const int64_t qv = a.ldv >> 2, qh = a.ldh >> 2;
    const int64_t nv = 2 * (int64_t)a.n * qv, nh = 2 * (int64_t)a.n * qh;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nv) {
        const int64_t r = e / qv, j = 4 * (e - r * qv);
        const int lv = (int)min(max((int64_t)a.V - j, (int64_t)0), (int64_t)4);
        const float* src = r < a.n ? a.lo + r * a.ldv : a.second + (r - a.n) * a.ldv;
        *reinterpret_cast<float4*>(a.V2 + r * a.ldv + j) = load_live(src + j, lv);
    } else if (e < nv + nh) {
        const int64_t f = e - nv;
        const int64_t r = f / qh, j = 4 * (f - r * qh);
        const int lv = (int)min(max((int64_t)a.H - j, (int64_t)0), (int64_t)4);
        float4 v;
        if (r < a.n) {
            v = load_live(a.hi + r * a.ldh + j, lv);
        } else {
            v = load_live(a.neg + (r - a.n) * a.ldh + j, lv);
            v = make_float4(lv > 0 ? -v.x : 0.f, lv > 1 ? -v.y : 0.f, lv > 2 ? -v.z : 0.f, lv > 3 ? -v.w : 0.f);
        }
        *reinterpret_cast<float4*>(a.P2 + r * a.ldh + j) = v;
    }
}

__global__ __launch_bounds__(UD_COST_NT) void updown_cost_kernel(UpdownCostArgs a)
{
    __shared__ float red[UD_COST_NT / 64];
    const int64_t total = (int64_t)a.n * a.V;
    float t = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * UD_COST_NT + threadIdx.x; e < total; e += (int64_t)a.G * UD_COST_NT) {
        const int64_t b = e / a.V, i = e - b * a.V;
        const float x = a.x[b * a.ldv + i], p = a.pre[b * a.ldv + i];
        if (a.gauss) { const float d = x - p; t += 0.5f * d * d; }
        else t += x * softplusf_(-p) + (1.0f - x) * softplusf_(p);
    }
    const float s = block_sum(t, red);
    if (threadIdx.x == 0) a.cost_partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(UD_COST_NT) void updown_cost_finish_kernel(const float* partials, int n, float scale, float* cost_out)
{
    __shared__ double run[UD_COST_NT];
    const int per = (n + UD_COST_NT - 1) / UD_COST_NT;       // contiguous ascending runs, then the runs in ascending order
    const int k0 = min((int)threadIdx.x * per, n), k1 = min(k0 + per, n);
    double s = 0.0;
    for (int k = k0; k < k1; ++k) s += (double)partials[k];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < UD_COST_NT; ++k) t += run[k];
        cost_out[0] = (float)(t * (double)scale);
    }
}

template <int BQ, int NCH>
hipError_t launch_updown_gen_t(const UpdownGenArgs& a, int lds, hipStream_t s)
{
    auto kern = updown_gen_kernel<BQ, NCH>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (UD_MAXB * UD_MAX_LDH + UD_MAX_RPW * UD_MAXB + UD_NT / 64) * 4);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.G), dim3(UD_NT), lds, s, a);
    return hipGetLastError();
}

template <int BQ, int NCH>
hipError_t launch_updown_gen_grouped_t(const UpdownGenGroupedArgs& a, int lds, hipStream_t s)
{
    auto kern = updown_gen_grouped_kernel<BQ, NCH>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           UD_GROUPED_MAX_LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.g.G), dim3(UD_NT), lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_updown_gen_grouped(const UpdownGenGroupedArgs& q, const UpdownGeom& t, hipStream_t s)
{
    const UpdownGenArgs& a = q.g;
    if (a.n < 1 || a.n > t.Bq || a.Bq != t.Bq || a.rpw != t.rpw || a.G != t.G || a.G != (a.V + a.rpw - 1) / a.rpw ||
        a.ldh > UD_MAX_LDH || a.ldh > 256 * t.nch || a.rpw > UD_MAX_RPW || a.gauss != 0 ||
        t.lds != (t.Bq * (int)a.ldh + 2 * (t.rpw + UD_GROUP_SLACK) * t.Bq + 2 * (UD_NT / 64)) * 4 || t.lds > UD_GROUPED_MAX_LDS ||
        !q.group_start || q.n_groups < 1 || q.span_lo < 0 || q.span_lo >= q.span_hi || q.span_hi > a.V ||
        q.n_groups > (q.span_hi - q.span_lo) / 2)
        return hipErrorInvalidValue;
#define UD_CASE(BQ)                                                                          \
    case BQ: return t.nch == 1 ? launch_updown_gen_grouped_t<BQ, 1>(q, t.lds, s) : launch_updown_gen_grouped_t<BQ, 2>(q, t.lds, s)
    switch (t.Bq) {
        UD_CASE(4);
        UD_CASE(8);
        UD_CASE(12);
        UD_CASE(16);
        UD_CASE(20);
        UD_CASE(24);
        UD_CASE(28);
        UD_CASE(32);
    }
#undef UD_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_updown_gen(const UpdownGenArgs& a, const UpdownGeom& t, hipStream_t s)
{
    if (a.n < 1 || a.n > t.Bq || a.Bq != t.Bq || a.rpw != t.rpw || a.G != t.G || a.G != (a.V + a.rpw - 1) / a.rpw ||
        a.ldh > UD_MAX_LDH || a.ldh > 256 * t.nch || a.rpw > UD_MAX_RPW || t.lds != (t.Bq * (int)a.ldh + t.rpw * t.Bq + UD_NT / 64) * 4)
        return hipErrorInvalidValue;
#define UD_CASE(BQ)                                                                          \
    case BQ: return t.nch == 1 ? launch_updown_gen_t<BQ, 1>(a, t.lds, s) : launch_updown_gen_t<BQ, 2>(a, t.lds, s)
    switch (t.Bq) {
        UD_CASE(4);
        UD_CASE(8);
        UD_CASE(12);
        UD_CASE(16);
        UD_CASE(20);
        UD_CASE(24);
        UD_CASE(28);
        UD_CASE(32);
    }
#undef UD_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_updown_stack(const UpdownStackArgs& a, hipStream_t s)
{
    if (a.n < 1 || a.V < 1 || a.H < 1 || a.ldv < a.V || a.ldh < a.H || (a.ldv & 3) || (a.ldh & 3)) return hipErrorInvalidValue;
    const int64_t items = 2 * (int64_t)a.n * ((a.ldv + a.ldh) >> 2);
    hipLaunchKernelGGL(updown_stack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_updown_cost(const UpdownCostArgs& a, hipStream_t s)
{
    if (a.n < 1 || a.V < 1 || a.G < 1 || a.G > UD_COST_MAXG || a.ldv < a.V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(updown_cost_kernel, dim3((unsigned)a.G), dim3(UD_COST_NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_updown_cost_finish(const float* partials, int n, float scale, float* cost_out, hipStream_t s)
{
    if (n < 1 || !partials || !cost_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(updown_cost_finish_kernel, dim3(1), dim3(UD_COST_NT), 0, s, partials, n, scale, cost_out);
    return hipGetLastError();
}

}  // namespace mdbn

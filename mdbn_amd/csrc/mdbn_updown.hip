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

}  // namespace

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

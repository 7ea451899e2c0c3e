// What the samplers of a trained layer share around the passes of mdbn_small_passes.h (mdbn_ais.hip: annealed importance
// sampling, free and under a clamp; mdbn_clamp.hip: clamped Gibbs sampling; mdbn_temper.hip: parallel
// tempering): the staging of a one-launch kernel's LDS image, the draws of the tempered family b_beta = b_A + beta (b - b_A)
// and the fixed-order sums.  Each is stated once because the samplers must agree bit for bit -- with each other, between their
// two paths and across the cuts of a run.  Included by those three sources only, after mdbn_small_passes.h.
#pragma once
#include "mdbn_device.h"
#include "mdbn_small_passes.h"

namespace mdbn {

namespace {

// ---- staging of a one-launch kernel (every thread of the SM_NT calls; the caller's barrier follows)
// W image [Vp][ldw]: rows >= V and columns >= ldh zero, + the slack behind the last row
__device__ __forceinline__ void sm_stage_w(lds_f* Wl, const SmallLayout& L, const float* W, int V, int64_t ldh, int tid)
{
    const int q4w = L.ldw >> 2, q4 = (int)(ldh >> 2);
    const int total = L.Vp * q4w + 4;
    for (int e = tid; e < total; e += SM_NT) {
        const int r = e / q4w, c4 = e - r * q4w;
        sf32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (r < V && c4 < q4) w = *reinterpret_cast<const sf32x4*>(W + (int64_t)r * ldh + 4 * c4);
        *(lds_f4*)(Wl + 4 * e) = w;
    }
}

// a bias row of n values on its n64 columns (the pad columns zero)
__device__ __forceinline__ void sm_stage_bias(lds_f* dst, const float* bias, int n64, int n, int tid)
{
    if (tid < n64) dst[tid] = tid < n ? bias[tid] : 0.f;
}

// the visible bias of the tempered family as the pair b_A, b - b_A
__device__ __forceinline__ void sm_stage_bias_pair(lds_f* bAl, lds_f* dbl, const float* vbias, const float* base_vbias, int V64, int V, int tid)
{
    if (tid < V64) {
        const float bA = tid < V ? base_vbias[tid] : 0.f, b = tid < V ? vbias[tid] : 0.f;
        bAl[tid] = bA; dbl[tid] = b - bA;
    }
}

// a 4-row operand buffer of the passes, pad columns included
__device__ __forceinline__ void sm_zero_rows(lds_f* buf, int pitch, int tid)
{
    for (int i = tid; i < SM_ROWS * pitch; i += SM_NT) buf[i] = 0.f;
}

// ---- sums in a fixed order
__device__ __forceinline__ float wave_sum(float x)       // every lane of the wave active; the same tree in every call
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// the four row sums of a workgroup of NT threads: wave by wave through red[4][NT / 64], the waves in ascending order;
// every thread leaves with all four (pt_visible_kernel, where four threads need one sum each, keeps a tail of its own)
template <int NT>
__device__ __forceinline__ void rows4_block_sum(float (&acc)[4], float* red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = wave_sum(acc[e]);
        if (lane == 0) red[e * (NT / 64) + wave] = t;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = 0.f;
        for (int w = 0; w < NT / 64; ++w) t += red[e * (NT / 64) + w];
        acc[e] = t;
    }
}

// ---- draws
__device__ __forceinline__ float box_muller(float u1, float u2)     // N(0, 1) from two philox_u01 uniforms (never 0)
{
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// the tempered visible pre-activation b_A + beta (b - b_A) + beta m of one (row, column)
__device__ __forceinline__ float tempered_pre_v(float beta, float m, float bA, float db)
{
    return fmaf(beta, m, fmaf(beta, db, bA));
}

// ---- the category draw of a softmax group of K columns (the arithmetic of group_softmax_kernel, mdbn_groups.hip), from its
// tempered pre-activations x_c:  mx = max_c x_c,  e_c = __expf(x_c - mx),  Z = sum_c e_c (ascending c, f32),
// mean_c = e_c / Z (correctly rounded),  C_c = the running f32 sum of the means;  the category is the first c with u < C_c and
// the last one when none qualifies.  C never falls (a sum of non-negative terms, rounded to nearest), so column c is the
// drawn one exactly when u >= C_{c-1} (C_{-1} = 0) and (u < C_c or c = K - 1): a thread that owns one column decides its
// own entry from the two sums (ais_small_kernel), a thread that owns the group walks it (group_draw, the general path).
// Both forms add the same operands in the same order.
__device__ __forceinline__ float group_exp(float x, float mx) { return __expf(x - mx); }
__device__ __forceinline__ float group_mean(float e, float Z) { return __fdiv_rn(e, Z); }
__device__ __forceinline__ float group_entry(float u, float C_before, float C, bool last)
{
    return !(u < C_before) && (u < C || last) ? 1.0f : 0.0f;
}

// one group of a 4-row block by one thread in three walks (max, Z, means): x(c, e) = the pre-activation of category c in row e,
// out(c, e, v) takes the 0 / 1 entry; K has no register cost.  The four rows go side by side through every walk -- their loads
// do not depend on each other, so a walk waits for memory once per category, not once per (category, row); each row's sums
// are its own, in ascending c.
// group_draw_mean: out(c, e, v, mean) also takes mean_c (the clamped chain keeps it).
template <class X, class Out>
__device__ __forceinline__ void group_draw_mean(int K, const float (&u)[4], X&& x, Out&& out)
{
    float mx[4], Z[4] = {0.f, 0.f, 0.f, 0.f}, cum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) mx[e] = x(0, e);
    for (int c = 1; c < K; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], x(c, e));
    }
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Z[e] += group_exp(x(c, e), mx[e]);
    }
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float before = cum[e];
            const float mean = group_mean(group_exp(x(c, e), mx[e]), Z[e]);
            cum[e] += mean;
            out(c, e, group_entry(u[e], before, cum[e], c == K - 1), mean);
        }
    }
}

template <class X, class Out>
__device__ __forceinline__ void group_draw(int K, const float (&u)[4], X&& x, Out&& out)
{
    group_draw_mean(K, u, x, [&](int c, int e, float v, float) { out(c, e, v); });
}

// v | h for one (4-row group, column), every row at its own beta: pre = b_A + beta (b - b_A) + beta m, then the draw.
// `s` receives the column's share of s1.
template <bool GAUSS>
__device__ __forceinline__ void tempered_draw_v(const PhiloxKey& key, uint64_t grow0, int col, const float (&beta)[4], float bA, float db,
                                                const float (&m)[4], const bool (&ok)[4], float (&v)[4], float (&pre)[4], float (&s)[4])
{
    uint32_t wa[4], wb[4] = {0u, 0u, 0u, 0u};
    philox_rows4(key, 0u, grow0, (uint32_t)col, wa);
    if (GAUSS) philox_rows4(key, MDBN_NORMAL_BIT, grow0, (uint32_t)col, wb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pre[e] = tempered_pre_v(beta[e], m[e], bA, db);
        if (GAUSS) {
            const float z = box_muller(philox_u01(wa[e]), philox_u01(wb[e]));
            v[e] = ok[e] ? pre[e] + z : 0.f;
            s[e] = ok[e] ? (v[e] - bA) * db : 0.f;
        } else {
            v[e] = ok[e] && philox_u01(wa[e]) < sigmoidf_(pre[e]) ? 1.0f : 0.0f;
            s[e] = v[e] * db;
        }
    }
}

// h | v for one (4-row group, column): p = sigmoid(beta a), a = pre-activation (c included); without `draw` h = 0 and no
// uniforms are generated
__device__ __forceinline__ void tempered_draw_h(const PhiloxKey& key, uint64_t grow0, int col, const float (&beta)[4], const float (&a)[4],
                                                const bool (&ok)[4], bool draw, float (&h)[4], float (&p)[4])
{
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (draw) philox_rows4(key, 0u, grow0, (uint32_t)col, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[e] = sigmoidf_(beta[e] * a[e]);
        h[e] = draw && ok[e] && philox_u01(w[e]) < p[e] ? 1.0f : 0.0f;
    }
}

// one hidden unit's share of l(beta_partner) - l(beta_own)
__device__ __forceinline__ float softplus_gap(float a, float b_own, float b_partner)
{
    return softplusf_(b_partner * a) - softplusf_(b_own * a);
}

}  // namespace

}  // namespace mdbn

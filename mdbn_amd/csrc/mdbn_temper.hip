// Parallel tempering (replica exchange; Desjardins et al. 2010, Cho et al. 2010) of a trained RBM / GRBM on gfx950 / MI355X:
// M ladders of R Gibbs chains at the inverse temperatures 0 <= beta_0 < ... < beta_{R-1} = 1 of the tempered family of
// mdbn_ais.hip (base-rate visible bias b_A, b_beta = b_A + beta (b - b_A)), with swaps between neighbouring temperatures.
//
//   joint at beta:  log p_beta(v, h) = beta (v W h + c h) + { b_beta . v  |  -|v - b_beta|^2 / 2 }
//   row m R + s = slot s of ladder m;  rank[m][s] = the temperature index the slot holds (swaps exchange ranks, never states)
//   sweep t (run step s = rng.step), every row at the beta of its rank:
//     1. v ~ sigmoid(b_beta + beta h W^T)  |  b_beta + beta h W^T + N(0, 1)                                  (step s + 3t)
//     2. a = v W + c;  l(beta') = sum_j softplus(beta' a_j) + { v . b_beta' | -|v - b_beta'|^2 / 2 }
//     3. rank pairs (rho, rho + 1), rho = sweep0 + t (mod 2): accept iff log u < l_i(beta_j) + l_j(beta_i) - l_i(beta_i)
//        - l_j(beta_j), u addressed by (ladder, rho) alone                                                  (step s + 3t + 1)
//     4. h ~ sigmoid(beta a) at the rank after the swap                                                     (step s + 3t + 2)
//   t >= burn_in: v_sum[m] += the beta = 1 mean of the slot that holds rank R - 1 when it draws v (sigmoid(b + h W^T) | b + h W^T),
//                 h_sum[m] += sigmoid(a) of the slot that holds rank R - 1 when it draws h                  (float32, in sweep order)
// The acceptance difference is formed with the regrouping of mdbn_ais.hip: per row the float32 sums
//   hsum = sum_j softplus(beta_partner a_j) - softplus(beta_own a_j),   s1 = sum_i (v_i - [Gaussian] b_A,i) (b - b_A)_i
// and  delta = hsum_lo + hsum_hi + (beta_hi - beta_lo) (s1_lo - s1_hi)  in double (the Gaussian |b - b_A|^2 terms of the two
// rows cancel).  Both paths call tempered_draw_v, tempered_draw_h and softplus_gap of mdbn_sampler_kit.h and pt_swap_accept
// below: the uniforms, their addressing and the decision are stated once.
//
// The works (log Z from the ladder).  The same four sums are the two halves of a bridge between neighbouring
// temperatures: for the attempted pair (rho, rho + 1) held by the slots i / j, with db = beta_hi - beta_lo, g = |b - b_A|^2,
//   d_fwd = l_i(beta_hi) - l_i(beta_lo) = hsum_i + db s1_i - [Gaussian] (beta_hi^2 - beta_lo^2) g / 2
//   d_rev = l_j(beta_lo) - l_j(beta_hi) = hsum_j - db s1_j + [Gaussian] (beta_hi^2 - beta_lo^2) g / 2
// in double (pt_works; g in double from the float32 differences, pt_gnorm_wave).  From sweep burn_in on, zacc[m][rho] =
// {m_f, s_f, m_r, s_r} keeps sum exp(d) per direction as a running maximum m and s = sum exp(d - m) (pt_z_add: s in double,
// the two exponentials float32); the caller starts it at (-inf, 0) and it is in-and-out like the rank map.  trace_work taps
// (d_fwd, d_rev) of every sweep (NaN: the pair was not tried).  Neither consumes a random number nor touches a decision.
//
// Softmax groups (mdbn_pt_run_grouped): a visible layer that holds a span of one-hot groups between Bernoulli columns
// (mdbn_groups.hip).  On one-hot rows log p*_beta(v) is the Bernoulli expression, so the swap decision, the works, the hidden
// draw, the rank map, the counts and the cuts are the plain run's; only the visible draw of a group changes -- v ~
// softmax_c(x_c) over the group's tempered pre-activations at the beta of the row's rank, ONE uniform per (replica row,
// group): the Philox word of the group's first column at step s + 3t, draw 0, by the group draw of mdbn_sampler_kit.h -- and
// with it the beta = 1 mean that v_sum takes from the top-rank row: the group's softmax mean.  s1 gets v_c (b - b_A)_c.
//
// pt_small_kernel (LDS-resident layers, R a multiple of 4): W staged once into the workgroup's LDS; a workgroup owns whole
// ladders, the R rows of h and a stay in LDS, a sweep runs R / 4 four-row slabs through sm_down / sm_up of
// mdbn_small_passes.h, the swap phase reads the per-row sums from LDS and exchanges ranks there.  Nothing crosses a workgroup.
// pt_visible_kernel / pt_swap_hidden_kernel (any shape): the per-sweep epilogues around the library's propdown / propup GEMMs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_device.h"
#include "mdbn_small.h"
#include "mdbn_small_passes.h"
#include "mdbn_sampler_kit.h"
#include "mdbn_temper.h"
#include "mdbn_groups.h"                    // MDBN_GROUP_MAX and the unit map the grouped visible kernel shares

namespace mdbn {

namespace {

typedef __attribute__((address_space(3))) int lds_i;
typedef __attribute__((address_space(3))) double lds_d;

// the rank a row of rank `rho` is paired with in a sweep of parity `par` (pairs (r, r + 1), r = par mod 2), or -1
__device__ __forceinline__ int pt_partner(int rho, int par, int R)
{
    const int p = ((rho ^ par) & 1) == 0 ? rho + 1 : rho - 1;
    return p >= 0 && p < R ? p : -1;
}

// the swap of the ranks (rho, rho + 1) of ladder `ladder`: log u < delta.  key.step = the sweep's swap step.
__device__ __forceinline__ bool pt_swap_accept(const PhiloxKey& key, uint64_t ladder, int rho, float hsum_lo, float hsum_hi,
                                               float s1_lo, float s1_hi, float b_lo, float b_hi)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)rho, (uint32_t)(ladder >> 2), 0u, key.step, key.k0, key.k1, w);
    const uint32_t ph = (uint32_t)(ladder & 3);
    const uint32_t word = ph == 0 ? w[0] : ph == 1 ? w[1] : ph == 2 ? w[2] : w[3];
    const double delta = (double)hsum_lo + (double)hsum_hi + ((double)b_hi - (double)b_lo) * ((double)s1_lo - (double)s1_hi);
    return (double)logf(philox_u01(word)) < delta;
}

// the works of the pair (rho, rho + 1) from the row sums of its swap; gq = (beta_hi^2 - beta_lo^2) g / 2 or 0 (Bernoulli)
__device__ __forceinline__ void pt_works(float hsum_lo, float hsum_hi, float s1_lo, float s1_hi, float b_lo, float b_hi, double gq,
                                         double& d_fwd, double& d_rev)
{
    const double db = (double)b_hi - (double)b_lo;
    d_fwd = (double)hsum_lo + db * (double)s1_lo - gq;
    d_rev = (double)hsum_hi - db * (double)s1_hi + gq;
}

__device__ __forceinline__ double pt_gq(float b_lo, float b_hi, double g)
{
    return 0.5 * ((double)b_hi * (double)b_hi - (double)b_lo * (double)b_lo) * g;
}

// sum exp(d) as (m, s): m' = max(m, d), s = s exp(m - m') + exp(d - m'); from (-inf, 0) the first work gives (d, 1)
__device__ __forceinline__ void pt_z_add(double& m, double& s, double d)
{
    const double m2 = d > m ? d : m;
    s = s * (double)expf((float)(m - m2)) + (double)expf((float)(d - m2));
    m = m2;
}

// |b - b_A|^2 by one whole wave: lane l sums the squares of the columns l, l + 64, ... in double, then the tree of wave_sum.
// `db(i)` = the float32 difference of column i < n.  Both paths take it, so both hold the same g.
template <class F>
__device__ __forceinline__ double pt_gnorm_wave(int n, int lane, F db)
{
    double t = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double d = (double)db(i);
        t += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}

// what a launcher asks of the groups: none, or a Bernoulli layer whose span lies inside the row (the rule of launch_ais_visible)
bool pt_groups_ok(const AisGroups& g, int V, int gauss)
{
    if (!g.on) return g.n_groups == 0;
    return !gauss && g.n_groups >= 0 && (g.n_groups == 0 || g.group_start) && g.span_lo >= 0 && g.span_lo <= g.span_hi &&
           g.span_hi <= V && (g.n_groups == 0) == (g.span_lo == g.span_hi) && g.n_groups <= g.span_hi - g.span_lo;
}

}  // namespace

// Z: the variants of mdbn_pt_run_z (the works; their tap rides with TRACE).  The Bernoulli variant without taps is held to
// the 128 VGPRs of two workgroups per CU, which pt_small_preferred counts on (127, no scratch; unbounded the compiler takes 129
// and a sweep at 100 -> 24 with 512 ladders costs 43 instead of 24 us); the bound 1 leaves the other variants as they were.
// GROUPS (mdbn_pt_run_grouped): a thread whose column lies in a softmax group leaves the slab's four tempered pre-activations
// in PX instead of drawing; after the pass's closing barrier every thread takes its group's maximum and writes its own e_c into
// EX, forms Z and its mean, then the running sum up to its own column and decides its own 0 / 1 entry (the group draw of
// mdbn_sampler_kit.h; ais_small_kernel).  PX / EX are small_layout's oX0 / oXb, which the plain kernel leaves unused, so
// pt_layout -- and pt_small_ok -- serve both.  The variants without taps are held to 128 VGPRs like the Z one.
template <bool GAUSS, bool TRACE, bool Z = false, bool GROUPS = false>
__global__ __launch_bounds__(SM_NT, ((Z || GROUPS) && !GAUSS && !TRACE) ? 4 : 1) void pt_small_kernel(PtSmallArgs a)
{
    static_assert(!GROUPS || !GAUSS, "softmax groups: a Bernoulli layer");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const SmallLayout& L = a.L;
    const PtLayout& P = a.P;
    lds_f* const lds = (lds_f*)sm;
    lds_f* const Wl = lds + L.oW;
    lds_f* const PX = lds + L.oX0;          // (groups) [V64][4] tempered pre-activations x_c of the group columns, then their means
    lds_f* const X = lds + L.oXa;           // [4][ldx] the slab's visible draw
    lds_f* const EX = lds + L.oXb;          // (groups) [V64][4] e_c = exp(x_c - max)
    lds_f* const part = lds + L.oPart;
    lds_f* const hbl = lds + L.oHb;         // c
    lds_f* const bAl = lds + L.oVb;         // b_A
    lds_f* const dbl = lds + L.oCsV;        // b - b_A
    lds_f* const Hs = lds + P.oHs;          // [R][ldhs] hidden samples of the ladder
    lds_f* const Al = lds + P.oA;           // [R][ldhs] a = v W + c
    lds_f* const redH = lds + P.oRedH;      // [R][8]
    lds_f* const redV = lds + P.oRedV;      // [R][8]
    lds_f* const betl = lds + P.oBeta;
    lds_i* const rk = (lds_i*)(lds + P.oRank);
    lds_i* const inv = (lds_i*)(lds + P.oInv);
    // [R - 1][4] the ladder's zacc: in small_layout's three 4-row hidden buffers (12 ldhs >= 864 floats; R - 1 <= 63 rows of 8),
    // which this kernel leaves unused.  Thread rho alone touches row rho: no barrier.  (In registers, as cnt is, the four doubles
    // are live across the passes: 140 VGPRs instead of 126, one workgroup per CU instead of two: DESIGN 3.7.)
    lds_d* const zl = (lds_d*)(lds + L.oHs);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int V = a.V, H = a.H, M = a.M, R = a.R;
    const int64_t ldv = a.ldv, ldh = a.ldh;
    const int nq = R / SM_ROWS;

    // ---- the LDS image: W, the biases, the betas, zeroed X
    sm_stage_w(Wl, L, a.W, V, ldh, tid);
    sm_stage_bias(hbl, a.hbias, L.H64, H, tid);
    sm_stage_bias_pair(bAl, dbl, a.vbias, a.base_vbias, L.V64, V, tid);
    if (tid < R) betl[tid] = a.betas[tid];
    sm_zero_rows(X, L.ldx, tid);

    // Both passes hand column `tid` to thread `tid` (propup: one column per thread; propdown: wave w owns tile w, tiles_dn <= 8),
    // so a thread keeps its column's two running sums in registers for the whole launch.
    const bool vlive = tid < V, hlive = tid < H;
    double g = 0.0;                                                      // (the deciding threads tid < R - 1 sit in wave 0)
    if (Z && GAUSS && wave == 0) g = pt_gnorm_wave(V, lane, [&](int i) { return a.vbias[i] - a.base_vbias[i]; });
    // ---- (groups) this thread's column belongs to the group [c0, c1) for the whole launch; c1 = c0: a Bernoulli column.
    // The last g with group_start[g] <= tid; the caller checked its host copy, the device copy is clamped to the span all the
    // same (ais_small_kernel), and a walk never leaves [c0, c1)
    int c0 = 0, c1 = 0;
    if constexpr (GROUPS) {
        const AisGroups& G = a.groups;
        if (tid >= G.span_lo && tid < G.span_hi && G.n_groups > 0) {
            int lo = 0, hi = G.n_groups - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (G.group_start[mid] <= tid) lo = mid; else hi = mid - 1;
            }
            c0 = min(max(G.group_start[lo], G.span_lo), tid);
            c1 = min(min(max(G.group_start[lo + 1], tid + 1), G.span_hi), c0 + MDBN_GROUP_MAX);
            if (c1 <= tid) c0 = c1 = 0;     // (a table the host copy does not describe: the column falls back to a Bernoulli unit)
        }
    }
    const bool grp = GROUPS && c1 > c0;
    const int cc = c0 | (c1 << 16);          // (one register for the launch: V64 <= 512)

    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        SM_SYNC();                                                       // (staging | the previous ladder's last readers are done)
        // ---- the ladder's state: h, the rank map and its inverse, the counts and the sums
        for (int i = tid; i < R * L.ldhs; i += SM_NT) {
            const int r = i / L.ldhs, col = i - r * L.ldhs;
            Hs[i] = col < H ? a.h[(int64_t)(m * R + r) * ldh + col] : 0.f;
        }
        if (tid < R) {
            const int rho = a.rank[m * R + tid];
            rk[tid] = rho;
            inv[rho] = tid;
        }
        float vacc = 0.f, hacc = 0.f;
        int cnt = 0;
        if (a.t0 > 0) {
            if (vlive) vacc = a.v_sum[(int64_t)m * ldv + tid];
            if (hlive) hacc = a.h_sum[(int64_t)m * ldh + tid];
            if (tid < R - 1) cnt = a.counts[m * (R - 1) + tid];
        }
        if (Z && a.zacc && tid < R - 1) {
            const double* z = a.zacc + ((int64_t)m * (R - 1) + tid) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) zl[4 * tid + k] = z[k];
        }
        SM_SYNC();

        for (int t = a.t0; t < a.t1; ++t) {
            const bool acc = t >= a.burn_in, out_v = t == a.t1 - 1;
            const int par = (int)((a.sweep0 + t) & 1);
            PhiloxKey kv = a.rng, ks = a.rng, kh = a.rng;
            kv.step = a.rng.step + (uint32_t)(3 * t);
            ks.step = a.rng.step + (uint32_t)(3 * t + 1);
            kh.step = a.rng.step + (uint32_t)(3 * t + 2);
            const bool okv[4] = {vlive, vlive, vlive, vlive}, okh[4] = {hlive, hlive, hlive, hlive};
            for (int q = 0; q < nq; ++q) {
                const int row0 = m * R + SM_ROWS * q;
                const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
                float bo[4], bp[4];
                bool top[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int rho = rk[SM_ROWS * q + e], pr = pt_partner(rho, par, R);
                    bo[e] = betl[rho];
                    bp[e] = pr >= 0 ? betl[pr] : bo[e];
                    top[e] = rho == R - 1;
                }
                if constexpr (GROUPS) {
                    // The visible draw in two parts (ais_small_kernel).  In the pass: a Bernoulli column draws as the plain kernel
                    // does, a group column leaves x_c in PX.  After the pass's closing barrier, every thread of the workgroup:
                    // e_c into EX -- ONE exponential per (row, column) --, barrier, Z and the column's mean, barrier, the running
                    // sum of the means up to the thread's own column and its 0 / 1 entry.  One uniform per (row, group): the Philox
                    // word of the group's first column.  Two barriers, whatever the groups; then X, redV, v and the taps.
                    // A column's entries wait in X, its share of s1 in its own EX slot (a Bernoulli column's is otherwise unused, a group
                    // column's has been read by then): nothing of a draw stays in a register across a pass or a barrier, and every
                    // column leaves through the one tail below.
                    sm_down(Hs + SM_ROWS * q * L.ldhs, Wl, L, wave, lane,
                            [&](const sf32x4& x, int col) {                // col == tid
                                asm volatile("" : "+v"(col));              // (as `me` below)
                                const float bA = bAl[col], db = dbl[col];
                                const float mm[4] = {x[0], x[1], x[2], x[3]};
                                if (grp) {
                                    *(lds_f4*)(PX + 4 * col) = sf32x4{tempered_pre_v(bo[0], mm[0], bA, db), tempered_pre_v(bo[1], mm[1], bA, db),
                                                                      tempered_pre_v(bo[2], mm[2], bA, db), tempered_pre_v(bo[3], mm[3], bA, db)};
                                } else {
                                    float v[4], pre[4], s[4];
                                    tempered_draw_v<false>(kv, grow0, col, bo, bA, db, mm, okv, v, pre, s);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        X[e * L.ldx + col] = v[e];
                                        if (acc && top[e] && vlive) vacc += sigmoidf_(pre[e]);
                                    }
                                    *(lds_f4*)(EX + 4 * col) = sf32x4{s[0], s[1], s[2], s[3]};
                                }
                            });
                    // (slab-local copies of the group's bounds and of the thread's slot: with the launch-wide values the compiler
                    //  hoists every walk's addresses and trip counts out of the sweeps, ~20 VGPRs held across the passes)
                    int gg = cc, me = tid;
                    asm volatile("" : "+v"(gg), "+v"(me));
                    const int g0 = gg & 0xffff, g1 = gg >> 16;
                    if (grp) {
                        sf32x4 mx = *(const lds_f4*)(PX + 4 * g0);
                        for (int c = g0 + 1; c < g1; ++c) {
                            const sf32x4 x = *(const lds_f4*)(PX + 4 * c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], x[e]);
                        }
                        const sf32x4 x = *(const lds_f4*)(PX + 4 * me);
                        *(lds_f4*)(EX + 4 * me) = sf32x4{group_exp(x[0], mx[0]), group_exp(x[1], mx[1]), group_exp(x[2], mx[2]), group_exp(x[3], mx[3])};
                    }
                    SM_SYNC();
                    if (grp) {
                        sf32x4 Zs = {0.f, 0.f, 0.f, 0.f};
                        for (int c = g0; c < g1; ++c) Zs += *(const lds_f4*)(EX + 4 * c);
                        const sf32x4 ex = *(const lds_f4*)(EX + 4 * me);
                        *(lds_f4*)(PX + 4 * me) = sf32x4{group_mean(ex[0], Zs[0]), group_mean(ex[1], Zs[1]), group_mean(ex[2], Zs[2]), group_mean(ex[3], Zs[3])};
                    }
                    SM_SYNC();
                    if (grp) {
                        uint32_t w[4];
                        philox_rows4(kv, 0u, grow0, (uint32_t)g0, w);
                        const float u[4] = {philox_u01(w[0]), philox_u01(w[1]), philox_u01(w[2]), philox_u01(w[3])};
                        sf32x4 before = {0.f, 0.f, 0.f, 0.f};
                        for (int c = g0; c < me; ++c) before += *(const lds_f4*)(PX + 4 * c);
                        const sf32x4 mean = *(const lds_f4*)(PX + 4 * me);
                        const float db = dbl[me];
                        sf32x4 s4;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float ve = group_entry(u[e], before[e], before[e] + mean[e], me == g1 - 1);
                            X[e * L.ldx + me] = ve;
                            s4[e] = ve * db;
                            if (acc && top[e]) vacc += mean[e];              // (the group's softmax mean at beta = 1)
                        }
                        *(lds_f4*)(EX + 4 * me) = s4;
                    }
                    if (tid < L.V64) {                                     // (whole waves: V64 is a multiple of 64; own slots: no barrier)
                        const int col = me;
                        const sf32x4 s4 = *(const lds_f4*)(EX + 4 * col);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float ts = wave_sum(s4[e]);
                            if (lane == 0) redV[(SM_ROWS * q + e) * 8 + (col >> 6)] = ts;
                        }
                        if (col < (int)ldv && (out_v || (TRACE && a.trace_v))) {
                            const float v[4] = {X[col], X[L.ldx + col], X[2 * L.ldx + col], X[3 * L.ldx + col]};
                            if (out_v) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) a.v[(int64_t)(row0 + e) * ldv + col] = v[e];
                            }
                            if (TRACE && a.trace_v) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) a.trace_v[((int64_t)t * M * R + row0 + e) * ldv + col] = v[e];
                            }
                        }
                    }
                    SM_SYNC();
                } else
                sm_down(Hs + SM_ROWS * q * L.ldhs, Wl, L, wave, lane,
                        [&](const sf32x4& x, int col) {                    // col == tid
                            const float bA = bAl[col], db = dbl[col];
                            const float mm[4] = {x[0], x[1], x[2], x[3]};
                            float v[4], pre[4], s[4];
                            tempered_draw_v<GAUSS>(kv, grow0, col, bo, bA, db, mm, okv, v, pre, s);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                X[e * L.ldx + col] = v[e];
                                if (acc && top[e] && vlive) vacc += GAUSS ? pre[e] : sigmoidf_(pre[e]);
                                const float ts = wave_sum(s[e]);
                                if (lane == 0) redV[(SM_ROWS * q + e) * 8 + (col >> 6)] = ts;
                            }
                            if (col < (int)ldv) {
                                if (out_v) {
#pragma unroll
                                    for (int e = 0; e < 4; ++e) a.v[(int64_t)(row0 + e) * ldv + col] = v[e];
                                }
                                if (TRACE && a.trace_v) {
#pragma unroll
                                    for (int e = 0; e < 4; ++e) a.trace_v[((int64_t)t * M * R + row0 + e) * ldv + col] = v[e];
                                }
                            }
                        });
                sm_up(X, Wl, L, part, wave, lane, [] {},
                      [&](const sf32x4& x, int col) {                      // col == tid
                          const float bias = hbl[col];
#pragma unroll
                          for (int e = 0; e < 4; ++e) {
                              const float pre = hlive ? x[e] + bias : 0.f;
                              Al[(SM_ROWS * q + e) * L.ldhs + col] = pre;
                              const float td = wave_sum(hlive ? softplus_gap(pre, bo[e], bp[e]) : 0.f);
                              if (lane == 0) redH[(SM_ROWS * q + e) * 8 + (col >> 6)] = td;
                          }
                      });
            }

            // ---- the swaps of this sweep: thread rho decides the pair (rho, rho + 1)
            int dec = -1;
            if (tid < R - 1 && ((tid ^ par) & 1) == 0) {
                const int i = inv[tid], j = inv[tid + 1];
                float hl = 0.f, hh = 0.f, sl = 0.f, sh = 0.f;
                for (int u = 0; u < L.tiles_up; ++u) { hl += redH[i * 8 + u]; hh += redH[j * 8 + u]; }
                for (int u = 0; u < L.tiles_dn; ++u) { sl += redV[i * 8 + u]; sh += redV[j * 8 + u]; }
                const uint64_t ladder = a.rng.row_offset / (uint64_t)R + (uint64_t)m;
                dec = pt_swap_accept(ks, ladder, tid, hl, hh, sl, sh, betl[tid], betl[tid + 1]) ? 1 : 0;
                if (dec) {
                    rk[i] = tid + 1; rk[j] = tid;
                    inv[tid] = j; inv[tid + 1] = i;
                    ++cnt;
                }
                if (Z) {
                    double df, dr;
                    pt_works(hl, hh, sl, sh, betl[tid], betl[tid + 1], GAUSS ? pt_gq(betl[tid], betl[tid + 1], g) : 0.0, df, dr);
                    if (TRACE && a.trace_work) {
                        double* tw = a.trace_work + (((int64_t)t * M + m) * (R - 1) + tid) * 2;
                        tw[0] = df; tw[1] = dr;
                    }
                    if (acc && a.zacc) {
#pragma unroll 1
                        for (int k = 0; k < 2; ++k) {                    // (one direction at a time: the registers of one)
                            double mk = zl[4 * tid + 2 * k], sk = zl[4 * tid + 2 * k + 1];
                            pt_z_add(mk, sk, k ? dr : df);
                            zl[4 * tid + 2 * k] = mk; zl[4 * tid + 2 * k + 1] = sk;
                        }
                    }
                }
            } else if (Z && TRACE && a.trace_work && tid < R - 1) {
                double* tw = a.trace_work + (((int64_t)t * M + m) * (R - 1) + tid) * 2;
                tw[0] = tw[1] = __builtin_nan("");
            }
            SM_SYNC();
            if (TRACE && a.trace_swaps && tid < R) {
                int* ts = a.trace_swaps + ((int64_t)t * M + m) * 2 * R;
                ts[tid] = rk[tid];
                ts[R + tid] = dec;
            }

            // ---- the hidden draw at the rank after the swap
            if (tid < L.H64) {
                const int col = tid;
                for (int q = 0; q < nq; ++q) {
                    const int row0 = m * R + SM_ROWS * q;
                    const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
                    float bn[4], pre[4], h[4], p[4];
                    bool top[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int rho = rk[SM_ROWS * q + e];
                        bn[e] = betl[rho];
                        top[e] = rho == R - 1;
                        pre[e] = Al[(SM_ROWS * q + e) * L.ldhs + col];
                    }
                    tempered_draw_h(kh, grow0, col, bn, pre, okh, true, h, p);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        Hs[(SM_ROWS * q + e) * L.ldhs + col] = h[e];
                        if (acc && top[e] && hlive) hacc += p[e];
                    }
                    if (TRACE && a.trace_h && col < (int)ldh) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) a.trace_h[((int64_t)t * M * R + row0 + e) * ldh + col] = h[e];
                    }
                }
            }
            SM_SYNC();
        }

        // ---- what the next launch (or the caller) reads
        const bool last = a.t1 == a.n;
        const float n_avg = (float)(a.n - a.burn_in);
        for (int i = tid; i < R * (int)ldh; i += SM_NT) {
            const int r = i / (int)ldh, col = i - r * (int)ldh;
            a.h[(int64_t)(m * R + r) * ldh + col] = Hs[r * L.ldhs + col];
        }
        if (tid < R) a.rank[m * R + tid] = rk[tid];
        if (tid < R - 1) a.counts[m * (R - 1) + tid] = cnt;
        if (Z && a.zacc && tid < R - 1) {
            double* z = a.zacc + ((int64_t)m * (R - 1) + tid) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = zl[4 * tid + k];
        }
        if (tid < (int)ldv) {
            a.v_sum[(int64_t)m * ldv + tid] = vacc;
            if (last && a.v_avg) a.v_avg[(int64_t)m * ldv + tid] = vacc / n_avg;
        }
        if (tid < (int)ldh) {
            a.h_sum[(int64_t)m * ldh + tid] = hacc;
            if (last && a.h_avg) a.h_avg[(int64_t)m * ldh + tid] = hacc / n_avg;
        }
    }
}

bool pt_small_ok(int64_t M, int64_t R, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh)
{
    if (M < 1 || R < 2 || R % SM_ROWS != 0 || R > PT_MAX_R || M * R >= (1ll << 31)) return false;
    if (!small_shape_ok(M * R, V, H, gauss) || !small_ld_ok(V, H, ldv, ldh)) return false;
    const SmallLayout L = small_layout((int)V, (int)H, gauss != 0);
    return L.tiles_dn <= SM_NW && pt_layout(L, (int)R).bytes <= SM_MAX_LDS;
}

// path = 0 takes the one-launch kernel only where it was measured to win: at least two workgroups per CU (the
// sweep of a ladder is a serial chain of R / 4 slab passes: a CU needs a second ladder to fill the gaps) and enough ladders to
// occupy the chip that way.  Elsewhere the general path, whose kernels spread all M R rows over the chip, is as fast or faster.
bool pt_small_preferred(int64_t M, int64_t R, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh)
{
    if (!pt_small_ok(M, R, V, H, gauss, ldv, ldh) || M < PT_SMALL_MIN_LADDERS) return false;
    return 2 * pt_layout(small_layout((int)V, (int)H, gauss != 0), (int)R).bytes <= SM_MAX_LDS;
}

int pt_default_cut(int64_t R)
{
    const int64_t slabs = (R + SM_ROWS - 1) / SM_ROWS;
    return (int)(PT_CUT / slabs > 1 ? PT_CUT / slabs : 1);
}

hipError_t launch_pt_small(const PtSmallArgs& a, hipStream_t s)
{
    if (!pt_small_ok(a.M, a.R, a.V, a.H, a.gauss, a.ldv, a.ldh) || a.t0 < 0 || a.t1 <= a.t0 || a.t1 > a.n || a.burn_in < 0 ||
        a.burn_in >= a.n)
        return hipErrorInvalidValue;
    if (!pt_groups_ok(a.groups, a.V, a.gauss)) return hipErrorInvalidValue;
    const SmallLayout L = small_layout(a.V, a.H, a.gauss != 0);
    const PtLayout P = pt_layout(L, a.R);
    const bool trace = a.trace_h || a.trace_v || a.trace_swaps || a.trace_work;      // (the tap of the works rides with the others)
    if (a.groups.on) {
        // the variants of a layer with softmax groups: 2 Z + TRACE (their dynamic-LDS limits are raised apart from the others)
        void (*const gkerns[4])(PtSmallArgs) = {pt_small_kernel<false, false, false, true>, pt_small_kernel<false, true, false, true>,
                                                pt_small_kernel<false, false, true, true>, pt_small_kernel<false, true, true, true>};
        static bool gattr_set[4] = {false, false, false, false};
        const int gv = ((a.zacc || a.trace_work) ? 2 : 0) | (trace ? 1 : 0);
        if (!gattr_set[gv]) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gkerns[gv]), hipFuncAttributeMaxDynamicSharedMemorySize, SM_MAX_LDS);
            if (e != hipSuccess) return e;
            gattr_set[gv] = true;
        }
        const dim3 ggrid(a.M < 1024 ? a.M : 1024), gblock(SM_NT);
        PtSmallArgs gk = a;
        gk.L = L; gk.P = P;
        hipLaunchKernelGGL(gkerns[gv], ggrid, gblock, P.bytes, s, gk);
        return hipGetLastError();
    }
    const int variant = (a.gauss ? 2 : 0) | (trace ? 1 : 0);
    void (*const kerns[4])(PtSmallArgs) = {pt_small_kernel<false, false>, pt_small_kernel<false, true>, pt_small_kernel<true, false>,
                                           pt_small_kernel<true, true>};
    // one workgroup per ladder; beyond 1024 ladders a workgroup loops (a ladder never leaves its workgroup)
    const dim3 grid(a.M < 1024 ? a.M : 1024), block(SM_NT);
    PtSmallArgs k = a;
    k.L = L; k.P = P;
    if (!a.zacc && !a.trace_work) return launch_small_variant(kerns, variant, grid, block, P.bytes, s, k);
    // the variants that record the works (their dynamic-LDS limits are raised apart from the four above)
    void (*const zkerns[4])(PtSmallArgs) = {pt_small_kernel<false, false, true>, pt_small_kernel<false, true, true>,
                                            pt_small_kernel<true, false, true>, pt_small_kernel<true, true, true>};
    static bool attr_set[4] = {false, false, false, false};
    if (!attr_set[variant]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(zkerns[variant]), hipFuncAttributeMaxDynamicSharedMemorySize, SM_MAX_LDS);
        if (e != hipSuccess) return e;
        attr_set[variant] = true;
    }
    hipLaunchKernelGGL(zkerns[variant], grid, block, P.bytes, s, k);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------
// General path.  pt_visible_kernel: a workgroup owns four consecutive replica rows (one Philox block), a thread walks the
// columns tid, tid + PT_NT, ...; the row sums of s1 are combined wave by wave in a fixed order.
// ----------------------------------------------------------------------------------
template <bool GAUSS>
__global__ __launch_bounds__(PT_NT) void pt_visible_kernel(PtStepArgs a)
{
    __shared__ float red[4 * (PT_NT / 64)];
    const int row0 = (int)blockIdx.x * 4, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = a.M * a.R;
    const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
    PhiloxKey key = a.rng;
    key.step = a.rng.step + (uint32_t)(3 * a.t);
    float beta[4];
    bool okr[4], top[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        okr[e] = row0 + e < rows;
        const int rho = okr[e] ? a.rank[row0 + e] : 0;
        beta[e] = a.betas[rho];
        top[e] = okr[e] && rho == a.R - 1;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int col = tid; col < (int)a.ldv; col += PT_NT) {
        const bool live = col < a.V;
        const float bA = live ? a.base_vbias[col] : 0.f, db = live ? a.vbias[col] - bA : 0.f;
        bool ok[4];
        float m[4], v[4], pre[4], s[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ok[e] = live && okr[e];
            m[e] = ok[e] ? a.pre[(int64_t)(row0 + e) * a.ldv + col] : 0.f;
        }
        tempered_draw_v<GAUSS>(key, grow0, col, beta, bA, db, m, ok, v, pre, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += s[e];
            if (!okr[e]) continue;
            a.v[(int64_t)(row0 + e) * a.ldv + col] = v[e];                 // (pad columns: zeros)
            if (a.trace_v) a.trace_v[(int64_t)(row0 + e) * a.ldv + col] = v[e];
            if (a.accumulate && top[e]) {                                  // (one row of a ladder holds the top rank: no other writer)
                const int64_t o = (int64_t)((row0 + e) / a.R) * a.ldv + col;
                const float t = a.v_sum[o] + (live ? (GAUSS ? pre[e] : sigmoidf_(pre[e])) : 0.f);
                a.v_sum[o] = t;
                if (a.last && a.v_avg) a.v_avg[o] = t / a.n_avg;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = wave_sum(acc[e]);
        if (lane == 0) red[e * (PT_NT / 64) + wave] = t;
    }
    __syncthreads();
    if (tid < 4 && okr[tid]) {
        float t = 0.f;
        for (int w = 0; w < PT_NT / 64; ++w) t += red[tid * (PT_NT / 64) + w];
        a.s1[row0 + tid] = t;
    }
}

// pt_visible_kernel<false> for a layer with softmax groups: a thread walks UNITS tid, tid + PT_NT, ... -- the unit map of
// GroupSoftmaxArgs (mdbn_groups.h), with the pad columns V .. ldv - 1 as Bernoulli units behind the span, written as zeros
// like the plain kernel writes them.  A Bernoulli unit is the plain kernel's column; a group is walked three times, its four
// replica rows side by side and every row at the beta of its own rank (group_draw_mean: max, Z, means), with x_c formed from
// a.pre on the fly, its uniform the Philox word of its first column.  The top-rank row adds the group's softmax mean to
// v_sum.  With n_groups = 0 a unit is a column and every sum has the plain kernel's operands in its order: the same bits.
__global__ __launch_bounds__(PT_NT) void pt_visible_grouped_kernel(PtStepArgs a)
{
    __shared__ float red[4 * (PT_NT / 64)];
    const int row0 = (int)blockIdx.x * 4, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = a.M * a.R;
    const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
    PhiloxKey key = a.rng;
    key.step = a.rng.step + (uint32_t)(3 * a.t);
    const AisGroups& G = a.groups;
    const int units = G.span_lo + G.n_groups + ((int)a.ldv - G.span_hi);
    float beta[4];
    bool okr[4], top[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        okr[e] = row0 + e < rows;
        const int rho = okr[e] ? a.rank[row0 + e] : 0;
        beta[e] = a.betas[rho];
        top[e] = okr[e] && rho == a.R - 1;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int unit = tid; unit < units; unit += PT_NT) {
        int c0, K = 0;                                   // first column; K = 0: a Bernoulli column
        if (unit < G.span_lo) {
            c0 = unit;
        } else if (unit < G.span_lo + G.n_groups) {
            const int g = unit - G.span_lo;
            // (the caller checked its host copy; the device copy is clamped to the span all the same)
            c0 = min(max(G.group_start[g], G.span_lo), G.span_hi - 1);
            K = min(min(max(G.group_start[g + 1], c0 + 1), G.span_hi) - c0, MDBN_GROUP_MAX);
        } else {
            c0 = G.span_hi + (unit - G.span_lo - G.n_groups);
        }
        if (K == 0) {
            const int col = c0;
            const bool live = col < a.V;
            const float bA = live ? a.base_vbias[col] : 0.f, db = live ? a.vbias[col] - bA : 0.f;
            bool ok[4];
            float m[4], v[4], pre[4], s[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ok[e] = live && okr[e];
                m[e] = ok[e] ? a.pre[(int64_t)(row0 + e) * a.ldv + col] : 0.f;
            }
            tempered_draw_v<false>(key, grow0, col, beta, bA, db, m, ok, v, pre, s);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e] += s[e];
                if (!okr[e]) continue;
                a.v[(int64_t)(row0 + e) * a.ldv + col] = v[e];             // (pad columns: zeros)
                if (a.trace_v) a.trace_v[(int64_t)(row0 + e) * a.ldv + col] = v[e];
                if (a.accumulate && top[e]) {                              // (one row of a ladder holds the top rank: no other writer)
                    const int64_t o = (int64_t)((row0 + e) / a.R) * a.ldv + col;
                    const float t = a.v_sum[o] + (live ? sigmoidf_(pre[e]) : 0.f);
                    a.v_sum[o] = t;
                    if (a.last && a.v_avg) a.v_avg[o] = t / a.n_avg;
                }
            }
            continue;
        }
        uint32_t w[4];
        philox_rows4(key, 0u, grow0, (uint32_t)c0, w);
        const float* bAp = a.base_vbias + c0;
        const float* bp = a.vbias + c0;
        int64_t off[4];
        float u[4], se[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            off[e] = (int64_t)(row0 + e) * a.ldv + c0;
            u[e] = philox_u01(w[e]);
        }
        group_draw_mean(K, u,
                        [&](int c, int e) {
                            const float bA = bAp[c];
                            return tempered_pre_v(beta[e], okr[e] ? a.pre[off[e] + c] : 0.f, bA, bp[c] - bA);
                        },
                        [&](int c, int e, float v, float mean) {
                            if (!okr[e]) return;
                            se[e] += v * (bp[c] - bAp[c]);
                            a.v[off[e] + c] = v;
                            if (a.trace_v) a.trace_v[off[e] + c] = v;
                            if (a.accumulate && top[e]) {                  // (the group's softmax mean at beta = 1)
                                const int64_t o = (int64_t)((row0 + e) / a.R) * a.ldv + c0 + c;
                                const float t = a.v_sum[o] + mean;
                                a.v_sum[o] = t;
                                if (a.last && a.v_avg) a.v_avg[o] = t / a.n_avg;
                            }
                        });
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += se[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = wave_sum(acc[e]);
        if (lane == 0) red[e * (PT_NT / 64) + wave] = t;
    }
    __syncthreads();
    if (tid < 4 && okr[tid]) {
        float t = 0.f;
        for (int w = 0; w < PT_NT / 64; ++w) t += red[tid * (PT_NT / 64) + w];
        a.s1[row0 + tid] = t;
    }
}

// pt_swap_hidden_kernel: a workgroup owns one ladder: the hidden share of l per row (one wave per row, a fixed tree), the
// swap decisions, the exchange of ranks, then the hidden draw of its R rows.
__global__ __launch_bounds__(PT_NT) void pt_swap_hidden_kernel(PtStepArgs a)
{
    extern __shared__ float psm[];
    const int R = a.R, m = (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const bet = psm;                  // [R]
    float* const hs = psm + R;               // [R]
    int* const rk = (int*)(psm + 2 * R);     // [R]
    int* const inv = rk + R;                 // [R]
    const int par = (int)((a.sweep0 + a.t) & 1);
    const int row0 = m * R;
    for (int s = tid; s < R; s += PT_NT) {
        bet[s] = a.betas[s];
        const int rho = a.rank[row0 + s];
        rk[s] = rho;
        inv[rho] = s;
    }
    __syncthreads();
    for (int s = wave; s < R; s += PT_NT / 64) {
        const int rho = rk[s], pr = pt_partner(rho, par, R);
        const float bo = bet[rho], bp = pr >= 0 ? bet[pr] : bo;
        float t = 0.f;
        for (int col = lane; col < a.H; col += 64) t += softplus_gap(a.pre[(int64_t)(row0 + s) * a.ldh + col], bo, bp);
        t = wave_sum(t);
        if (lane == 0) hs[s] = t;
    }
    __syncthreads();
    PhiloxKey ks = a.rng, kh = a.rng;
    ks.step = a.rng.step + (uint32_t)(3 * a.t + 1);
    kh.step = a.rng.step + (uint32_t)(3 * a.t + 2);
    int* const ts = a.trace_swaps;
    for (int rho = tid; rho < R; rho += PT_NT) {
        int dec = -1;
        if (rho < R - 1 && ((rho ^ par) & 1) == 0) {
            const int i = inv[rho], j = inv[rho + 1];
            const uint64_t ladder = a.rng.row_offset / (uint64_t)R + (uint64_t)m;
            dec = pt_swap_accept(ks, ladder, rho, hs[i], hs[j], a.s1[row0 + i], a.s1[row0 + j], bet[rho], bet[rho + 1]) ? 1 : 0;
            if (dec) {
                rk[i] = rho + 1; rk[j] = rho;
                a.counts[m * (R - 1) + rho] += 1;
            }
            if (a.zacc || a.trace_work) {
                double df, dr;
                pt_works(hs[i], hs[j], a.s1[row0 + i], a.s1[row0 + j], bet[rho], bet[rho + 1],
                         a.gauss ? pt_gq(bet[rho], bet[rho + 1], a.g[0]) : 0.0, df, dr);
                if (a.zacc && a.accumulate) {
                    double* z = a.zacc + ((int64_t)m * (R - 1) + rho) * 4;
                    double mf = z[0], sf = z[1], mr = z[2], sr = z[3];
                    pt_z_add(mf, sf, df); pt_z_add(mr, sr, dr);
                    z[0] = mf; z[1] = sf; z[2] = mr; z[3] = sr;
                }
                if (a.trace_work) {
                    double* tw = a.trace_work + ((int64_t)m * (R - 1) + rho) * 2;
                    tw[0] = df; tw[1] = dr;
                }
            }
        } else if (a.trace_work && rho < R - 1) {
            double* tw = a.trace_work + ((int64_t)m * (R - 1) + rho) * 2;
            tw[0] = tw[1] = __builtin_nan("");
        }
        if (ts) ts[(int64_t)m * 2 * R + R + rho] = dec;
    }
    __syncthreads();
    for (int s = tid; s < R; s += PT_NT) {
        a.rank[row0 + s] = rk[s];
        if (ts) ts[(int64_t)m * 2 * R + s] = rk[s];
    }
    const int groups = (R + 3) / 4, ldh = (int)a.ldh;
    for (int idx = tid; idx < groups * ldh; idx += PT_NT) {
        const int g = idx / ldh, col = idx - g * ldh;
        const bool live = col < a.H;
        float bn[4], pre[4], h[4], p[4];
        bool ok[4], top[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = 4 * g + e;
            const bool in = s < R;
            const int rho = in ? rk[s] : 0;
            ok[e] = in && live;
            bn[e] = bet[rho];
            top[e] = in && rho == R - 1;
            pre[e] = ok[e] ? a.pre[(int64_t)(row0 + s) * ldh + col] : 0.f;
        }
        tempered_draw_h(kh, a.rng.row_offset + (uint64_t)(row0 + 4 * g), col, bn, pre, ok, true, h, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = 4 * g + e;
            if (s >= R) continue;
            a.h[(int64_t)(row0 + s) * ldh + col] = h[e];                   // (pad columns: zeros)
            if (a.trace_h) a.trace_h[(int64_t)(row0 + s) * ldh + col] = h[e];
            if (a.accumulate && top[e]) {
                const int64_t o = (int64_t)m * ldh + col;
                const float t = a.h_sum[o] + (live ? p[e] : 0.f);
                a.h_sum[o] = t;
                if (a.last && a.h_avg) a.h_avg[o] = t / a.n_avg;
            }
        }
    }
}

// accepted[rho] = sum over the ladders of counts[m][rho] (integers: any order gives the same sum)
__global__ __launch_bounds__(64) void pt_counts_kernel(const int* counts, int M, int R, int* accepted)
{
    for (int rho = (int)(blockIdx.x * 64 + threadIdx.x); rho < R - 1; rho += (int)gridDim.x * 64) {
        int t = 0;
        for (int m = 0; m < M; ++m) t += counts[m * (R - 1) + rho];
        accepted[rho] = t;
    }
}

// g[0] = |b - b_A|^2 (one wave; the order of pt_small_kernel)
__global__ __launch_bounds__(64) void pt_gnorm_kernel(const float* vbias, const float* base_vbias, int V, double* g)
{
    const double t = pt_gnorm_wave(V, (int)threadIdx.x, [&](int i) { return vbias[i] - base_vbias[i]; });
    if (threadIdx.x == 0) g[0] = t;
}

hipError_t launch_pt_visible(const PtStepArgs& a, hipStream_t s)
{
    if (a.M < 1 || a.R < 2 || a.t < 0 || !pt_groups_ok(a.groups, a.V, a.gauss)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((int64_t)a.M * a.R + 3) / 4);
    if (a.groups.on) hipLaunchKernelGGL(pt_visible_grouped_kernel, dim3(blocks), dim3(PT_NT), 0, s, a);
    else if (a.gauss) hipLaunchKernelGGL((pt_visible_kernel<true>), dim3(blocks), dim3(PT_NT), 0, s, a);
    else hipLaunchKernelGGL((pt_visible_kernel<false>), dim3(blocks), dim3(PT_NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pt_swap_hidden(const PtStepArgs& a, hipStream_t s)
{
    if (a.M < 1 || a.R < 2 || a.R > PT_MAX_R_GENERAL || a.t < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_swap_hidden_kernel, dim3((unsigned)a.M), dim3(PT_NT), (size_t)a.R * 16, s, a);
    return hipGetLastError();
}

hipError_t launch_pt_gnorm(const float* vbias, const float* base_vbias, int V, double* g, hipStream_t s)
{
    hipLaunchKernelGGL(pt_gnorm_kernel, dim3(1), dim3(64), 0, s, vbias, base_vbias, V, g);
    return hipGetLastError();
}

hipError_t launch_pt_counts(const int* counts, int M, int R, int* accepted, hipStream_t s)
{
    hipLaunchKernelGGL(pt_counts_kernel, dim3((unsigned)((R - 1 + 63) / 64)), dim3(64), 0, s, counts, M, R, accepted);
    return hipGetLastError();
}

}  // namespace mdbn

// Annealed importance sampling (Salakhutdinov & Murray 2008) of a trained RBM / GRBM on gfx950 / MI355X: M independent
// chains annealed from a base-rate model (W = 0, c = 0, visible bias b_A) to the trained model through the inverse
// temperatures 0 = beta_0 < ... < beta_K = 1; log Z ~ log Z_A + log mean exp(log w).
//
//   a(v) = v W + c,  b_beta = b_A + beta (b - b_A)
//   temperature k = 1 .. K:  log w += sum_j softplus(beta_k a_j(v_k)) - softplus(beta_{k-1} a_j(v_k))
//                                     + (beta_k - beta_{k-1}) s1(v_k)  [- (beta_k^2 - beta_{k-1}^2) / 2 * sum_i (b - b_A)_i^2, Gaussian]
//                            s1(v) = sum_i (v_i - [Gaussian] b_A,i) (b - b_A)_i        (the bias term of log p*_beta, regrouped:
//                                     v . b_beta for Bernoulli, -|v - b_beta|^2 / 2 for Gaussian visibles, as a difference)
//                            k < K:  h ~ Bernoulli(sigmoid(beta_k a(v_k))),  m = h W^T,
//                                    v_{k+1} ~ Bernoulli(sigmoid(b_beta_k + beta_k m))  |  b_beta_k + beta_k m + N(0, 1)
// Products, softplus and row sums are float32; the per-chain log w is a double (one scalar add per chain and temperature).
// Random draws: rng.step = s: v_1 uses step s, the hidden draw of temperature k step s + 2 k - 1, its visible draw s + 2 k,
// draw index 0, the usual (column, global row >> 2) addressing -- so a run cut into several launches, the one-launch path and
// the general path all meet the same uniforms.
//
// The clamp (mdbn_ais_cond_run): part of the visible layer held at observed values -- the conditional partition function Z_r of
// the RBM over the free columns of data row r, whose hidden bias is the row's own c + v_O W_O; log p(v_F | v_O) = -F(v) - (bias
// term of the held columns) - log Z_r.  Chain m of the M = N C chains belongs to data row m / C.
//   a(v) over the WHOLE visible row (held columns at obs);  v := mask ? obs : v  after every visible draw (v_1 ~ p_0 included),
//   s1(v) and d2_r = sum_i (b - b_A)_i^2 over the FREE columns (of mask row r)
// A held column enters every sum as 0.f at its own place in the free run's tree, so with no held column the clamped kernels give
// the free run bit for bit; the Philox addressing is unchanged (a held column's uniform is drawn and not used).  CLAMP = false
// is the free run: no mask, no obs, one d2 for all chains.
//
// Softmax groups (mdbn_ais_run_grouped): a visible layer that holds a span of one-hot groups between Bernoulli columns
// (mdbn_groups.hip).  log p*_beta(v) is the Bernoulli expression on one-hot rows, so the weight update, the hidden draw, the
// double log w, the Philox steps and the hand-over of a cut run are the free run's; only the visible draw of a group column
// changes (v_1 ~ p_0 included): v ~ softmax_c(x_c) over the group's tempered pre-activations x_c, ONE uniform per (chain,
// group) -- the Philox word of the group's first column -- by the group draw of mdbn_sampler_kit.h, which both paths compose
// from the same float32 operations in the same order.  A Bernoulli column outside the span keeps its draw.
//
// Both (mdbn_ais_cond_run_grouped): a group is held or free as a WHOLE, by the mask entry at its FIRST column in the chain's
// mask row (the entries at its other columns are not read).  A held group's columns take obs as they are and enter s1 as 0.f,
// each at its own place; its uniform is drawn and not used.  A Bernoulli column keeps the clamp above.  With n_groups = 0 the
// run is mdbn_ais_cond_run's, with no held unit mdbn_ais_run_grouped's, bit for bit.
//
// ais_small_kernel (LDS-resident layers): the shape of small_cd_kernel -- W staged once into one CU's LDS, a workgroup owns
// four-chain slabs (one Philox block) and runs the whole loop over the temperatures on the exact-f32 4x4x1 MFMA passes of
// mdbn_small_passes.h.  No workgroup ever waits for, or exchanges anything with, another.  Both passes hand column `tid` to
// thread `tid`, so under the clamp a thread keeps the observed values and mask bits of its column for the slab's four chains (two
// data rows where C is no multiple of 4) in registers.
// ais_hidden_kernel / ais_visible_kernel (any shape): the per-temperature epilogues around the library's propup / propdown
// GEMMs; a workgroup owns a four-chain group and reduces its rows in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_device.h"
#include "mdbn_small.h"
#include "mdbn_small_passes.h"
#include "mdbn_sampler_kit.h"
#include "mdbn_ais.h"
#include "mdbn_groups.h"                    // MDBN_GROUP_MAX and the unit map the grouped visible kernel shares

namespace mdbn {

namespace {

// v_{k+1} | h_k for one (4-chain group, column): tempered_draw_v with every chain at the one beta of the temperature
template <bool GAUSS>
__device__ __forceinline__ void ais_draw_v(const PhiloxKey& key, uint64_t grow0, int col, float beta, float bA, float db,
                                           const float (&m)[4], const bool (&ok)[4], float (&v)[4], float (&s)[4])
{
    const float b4[4] = {beta, beta, beta, beta};
    float pre[4];
    tempered_draw_v<GAUSS>(key, grow0, col, b4, bA, db, m, ok, v, pre, s);
}

// h_k | v_k (tempered_draw_h at beta_k = b1) and the hidden share of the weight update for one (4-chain group, column);
// a = pre-activation (c included)
__device__ __forceinline__ void ais_draw_h(const PhiloxKey& key, uint64_t grow0, int col, float b1, float b0, bool draw,
                                           const float (&a)[4], const bool (&ok)[4], float (&h)[4], float (&d)[4])
{
    const float b4[4] = {b1, b1, b1, b1};
    float p[4];
    tempered_draw_h(key, grow0, col, b4, a, ok, draw, h, p);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = ok[e] ? softplus_gap(a[e], b0, b1) : 0.f;
}

// log w after one temperature (double: the increments are O(1 / K) of a total of hundreds of nats)
__device__ __forceinline__ double ais_logw_add(double lw, float hsum, float s1, float d2, float b1, float b0, bool gauss)
{
    const double B1 = (double)b1, B0 = (double)b0;
    lw += (double)hsum + (B1 - B0) * (double)s1;
    if (gauss) lw -= 0.5 * (B1 * B1 - B0 * B0) * (double)d2;
    return lw;
}

// the clamp of one (4-chain group, column): a held chain takes its observed value and leaves s1 alone
__device__ __forceinline__ void ais_clamp(const float (&ob)[4], const bool (&held)[4], float (&v)[4], float (&s)[4])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = held[e] ? ob[e] : v[e];
        s[e] = held[e] ? 0.f : s[e];
    }
}

// what a launcher asks of the clamp's description (both argument structs): whole data rows, one mask row or one per data row,
// and without a mask the shape of "one data row per chain"
template <class Args>
bool ais_clamp_ok(const Args& a)
{
    return a.M >= 1 && a.C >= 1 && a.M % a.C == 0 && (a.mask_rows == 1 || a.mask_rows == a.M / a.C) &&
           (a.mask != nullptr || (a.C == 1 && a.mask_rows == 1));
}

// ... and of the groups: none, or a Bernoulli layer, free or under a clamp, whose span lies inside the row (the rule of
// launch_group_softmax)
bool ais_groups_ok(const AisGroups& g, int V, int gauss)
{
    if (!g.on) return g.n_groups == 0;
    return !gauss && g.n_groups >= 0 && (g.n_groups == 0 || g.group_start) && g.span_lo >= 0 && g.span_lo <= g.span_hi &&
           g.span_hi <= V && (g.n_groups == 0) == (g.span_lo == g.span_hi) && g.n_groups <= g.span_hi - g.span_lo;
}

}  // namespace

template <bool GAUSS, bool TRACE, bool CLAMP, bool GROUPS = false>
__global__ __launch_bounds__(SM_NT) void ais_small_kernel(AisSmallArgs a)
{
    static_assert(!GROUPS || !GAUSS, "softmax groups: a Bernoulli layer");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const SmallLayout& L = a.L;
    lds_f* const lds = (lds_f*)sm;
    // small_layout's buffers under the roles they have here
    lds_f* const Wl = lds + L.oW;
    lds_f* const X = lds + L.oXa;           // [4][ldx] visible state v_k (after the clamp)
    lds_f* const PX = lds + L.oX0;          // (groups) [V64][4] tempered pre-activations x_c of the group columns, then their means
    lds_f* const EX = lds + L.oXb;          // (groups) [V64][4] e_c = exp(x_c - max): the Bernoulli layout's third row buffer
    lds_f* const Hs = lds + L.oHs;          // [4][ldhs] hidden sample h_k
    lds_f* const part = lds + L.oPart;
    lds_f* const hbl = lds + L.oHb;         // c
    lds_f* const bAl = lds + L.oVb;         // b_A
    lds_f* const dbl = lds + L.oCsV;        // b - b_A
    lds_f* const redH = lds + L.oM0;        // [4][8] per-wave row partials of the hidden share (one per 64-column tile)
    lds_f* const redV = redH + 32;          // [4][8] ... of s1
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int V = a.V, H = a.H, M = a.M, K = a.K;
    const int64_t ldv = a.ldv, ldh = a.ldh;
    const int nslabs = (M + SM_ROWS - 1) / SM_ROWS;

    // ---- the LDS image: W, the biases, zeroed row buffers
    sm_stage_w(Wl, L, a.W, V, ldh, tid);
    sm_stage_bias(hbl, a.hbias, L.H64, H, tid);
    sm_stage_bias_pair(bAl, dbl, a.vbias, a.base_vbias, L.V64, V, tid);
    sm_zero_rows(X, L.ldx, tid);
    sm_zero_rows(Hs, L.ldhs, tid);
    SM_SYNC();
    float d2 = 0.f;                          // sum_i (b - b_A)_i^2: every thread sums it in the same order (clamp: per slab, below)
    if (GAUSS && !CLAMP) {
        for (int i = lane; i < L.V64; i += 64) d2 += dbl[i] * dbl[i];
        d2 = wave_sum(d2);
    }
    // ---- (groups) this thread's column belongs to the group [c0, c1) for the whole launch; c1 = c0: a Bernoulli column.
    // The last g with group_start[g] <= tid; the caller checked its host copy, the device copy is clamped to the span all the
    // same (group_softmax_kernel), and a walk never leaves [c0, c1)
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

    for (int slab = blockIdx.x; slab < nslabs; slab += gridDim.x) {
        const int row0 = slab * SM_ROWS;
        const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
        bool ok[4];
        int64_t mrow[4];                     // (clamp) where the chain's mask row starts
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ok[e] = row0 + e < M;
            if constexpr (CLAMP) mrow[e] = a.mask_rows == 1 ? 0 : (int64_t)((row0 + e) / a.C) * ldv;
        }
        if (slab != (int)blockIdx.x) SM_SYNC();                        // (the previous slab's last readers are done)

        // ---- the clamp of this thread's column, in registers for the whole slab (a group column: held with its group, by the
        // mask entry at the group's first column; its observed value is its own)
        float ob[4] = {0.f, 0.f, 0.f, 0.f};
        bool held[4] = {false, false, false, false};
        if constexpr (CLAMP) {
            if (tid < V) {
                const int mcol = grp ? c0 : tid;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!ok[e]) continue;
                    held[e] = a.mask[mrow[e] + mcol] != 0.f;
                    ob[e] = a.obs[(int64_t)((row0 + e) / a.C) * ldv + tid];
                }
            }
            // d2 of the chain's mask row: the free run's sum (lane-strided, then the wave's tree) with a held column as 0.f.
            // Only the first wave needs it (thread e < 4 keeps chain e's log w).
            d2 = 0.f;
            if (GAUSS && wave == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = 0.f;
                    for (int i = lane; i < L.V64; i += 64) {
                        const bool free_col = !(ok[e] && i < V && a.mask[mrow[e] + i] != 0.f);
                        const float d = free_col ? dbl[i] : 0.f;
                        t += d * d;
                    }
                    t = wave_sum(t);
                    if (tid == e) d2 = t;
                }
            }
        }

        // a visible state goes into X; its share of s1 into redV (whole waves: V64 is a multiple of 64)
        auto put_v = [&](const float (&v)[4], const float (&s)[4], int col, float* trace) {
#pragma unroll
            for (int e = 0; e < 4; ++e) X[e * L.ldx + col] = v[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = wave_sum(s[e]);
                if (lane == 0) redV[e * 8 + (col >> 6)] = t;
            }
            if (TRACE && trace && col < (int)ldv) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ok[e]) trace[(int64_t)(row0 + e) * ldv + col] = v[e];
            }
        };
        // (groups) a visible draw in two parts.  group_x, in the place of the Bernoulli draw: the four tempered pre-activations
        // of a group column go into PX.  group_pick, every thread of the workgroup, after the barrier that follows: e_c into
        // EX -- ONE exponential per (chain, column) --, barrier, Z and the column's mean over x_c in PX, barrier, the running
        // sum of the means up to the thread's own column and its 0 / 1 entry (mdbn_sampler_kit.h: the group draw).  One uniform
        // per (chain, group): the Philox word of the group's first column.  Two barriers, whatever the groups.
        // PX and EX hold a column's four chains side by side ([column][4]: one 16-byte read per category serves all four).
        auto group_x = [&](float beta, const float (&m)[4], float bA, float db, int col) {
            *(lds_f4*)(PX + 4 * col) = sf32x4{tempered_pre_v(beta, m[0], bA, db), tempered_pre_v(beta, m[1], bA, db),
                                              tempered_pre_v(beta, m[2], bA, db), tempered_pre_v(beta, m[3], bA, db)};
        };
        auto group_pick = [&](const PhiloxKey& key, float (&v)[4], float (&s)[4]) {
            if (grp) {
                sf32x4 mx = *(const lds_f4*)(PX + 4 * c0);
                for (int c = c0 + 1; c < c1; ++c) {
                    const sf32x4 x = *(const lds_f4*)(PX + 4 * c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], x[e]);
                }
                const sf32x4 x = *(const lds_f4*)(PX + 4 * tid);
                *(lds_f4*)(EX + 4 * tid) = sf32x4{group_exp(x[0], mx[0]), group_exp(x[1], mx[1]), group_exp(x[2], mx[2]), group_exp(x[3], mx[3])};
            }
            SM_SYNC();
            if (grp) {
                sf32x4 Z = {0.f, 0.f, 0.f, 0.f};
                for (int c = c0; c < c1; ++c) Z += *(const lds_f4*)(EX + 4 * c);
                const sf32x4 ex = *(const lds_f4*)(EX + 4 * tid);
                *(lds_f4*)(PX + 4 * tid) = sf32x4{group_mean(ex[0], Z[0]), group_mean(ex[1], Z[1]), group_mean(ex[2], Z[2]), group_mean(ex[3], Z[3])};
            }
            SM_SYNC();
            if (grp) {
                uint32_t w[4];
                philox_rows4(key, 0u, grow0, (uint32_t)c0, w);
                const float db = dbl[tid];
                sf32x4 before = {0.f, 0.f, 0.f, 0.f};
                for (int c = c0; c < tid; ++c) before += *(const lds_f4*)(PX + 4 * c);
                const sf32x4 upto = before + *(const lds_f4*)(PX + 4 * tid);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = ok[e] ? group_entry(philox_u01(w[e]), before[e], upto[e], tid == c1 - 1) : 0.f;
                    s[e] = v[e] * db;
                }
            }
        };
        // ---- the chain's start: v_1 ~ p_0 (step s) under the clamp, or the state an earlier launch left
        double lw = 0.0;
        float v[4], s[4];                    // this thread's column of the visible state, from a draw to put_v
        if (tid < L.V64) {
            const int col = tid;
            const bool live = col < V;
            const float bA = bAl[col], db = dbl[col];
            const bool okc[4] = {ok[0] && live, ok[1] && live, ok[2] && live, ok[3] && live};
            if (a.k0 == 0) {
                const float m0[4] = {0.f, 0.f, 0.f, 0.f};
                if (grp) group_x(0.0f, m0, bA, db, col);
                else ais_draw_v<GAUSS>(a.rng, grow0, col, 0.0f, bA, db, m0, okc, v, s);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = okc[e] ? a.v_state[(int64_t)(row0 + e) * ldv + col] : 0.f;
                    s[e] = okc[e] ? (GAUSS ? (v[e] - bA) * db : v[e] * db) : 0.f;
                }
            }
            if constexpr (CLAMP && !GROUPS) ais_clamp(ob, held, v, s);
            if constexpr (!GROUPS) put_v(v, s, col, a.k0 == 0 ? a.trace_v : nullptr);
        }
        if constexpr (GROUPS) {
            if (a.k0 == 0) {
                SM_SYNC();
                group_pick(a.rng, v, s);
            }
            if (tid < L.V64) {                                         // (a group column has its v / s only now: the clamp follows the pick)
                if constexpr (CLAMP) ais_clamp(ob, held, v, s);
                put_v(v, s, tid, a.k0 == 0 ? a.trace_v : nullptr);
            }
        }
        if (a.k0 > 0 && tid < SM_ROWS && row0 + tid < M) lw = a.logw[row0 + tid];
        SM_SYNC();
        float s1 = 0.f;
        if (tid < SM_ROWS)
            for (int t = 0; t < L.tiles_dn; ++t) s1 += redV[tid * 8 + t];

        // ---- the temperatures of this launch (beta_{k+1} is requested one temperature ahead of its use)
        float b0 = a.betas[a.k0], b1 = a.betas[a.k0 + 1];
        for (int k = a.k0 + 1; k <= a.k1; ++k) {
            const float b_next = a.betas[min(k + 1, K)];
            const bool draw = k < K;
            PhiloxKey kh = a.rng, kv = a.rng;
            kh.step = a.rng.step + (uint32_t)(2 * k - 1);
            kv.step = a.rng.step + (uint32_t)(2 * k);
            sm_up(X, Wl, L, part, wave, lane, [] {},
                  [&](const sf32x4& x, int col) {
                      const bool live = col < H;
                      const float bias = hbl[col];
                      const bool okc[4] = {ok[0] && live, ok[1] && live, ok[2] && live, ok[3] && live};
                      const float pre[4] = {x[0] + bias, x[1] + bias, x[2] + bias, x[3] + bias};
                      float h[4], d[4];
                      ais_draw_h(kh, grow0, col, b1, b0, draw, pre, okc, h, d);
#pragma unroll
                      for (int e = 0; e < 4; ++e) Hs[e * L.ldhs + col] = h[e];
#pragma unroll
                      for (int e = 0; e < 4; ++e) {
                          const float t = wave_sum(d[e]);
                          if (lane == 0) redH[e * 8 + (col >> 6)] = t;
                      }
                      if (TRACE && a.trace_h && draw && col < (int)ldh) {
#pragma unroll
                          for (int e = 0; e < 4; ++e)
                              if (ok[e]) a.trace_h[((int64_t)(k - 1) * M + row0 + e) * ldh + col] = h[e];
                      }
                  });
            if (tid < SM_ROWS) {
                float hsum = 0.f;
                for (int t = 0; t < L.tiles_up; ++t) hsum += redH[tid * 8 + t];
                lw = ais_logw_add(lw, hsum, s1, d2, b1, b0, GAUSS);
            }
            if (draw) {
                sm_down(Hs, Wl, L, wave, lane,
                        [&](const sf32x4& x, int col) {                // col == tid: ob / held are this column's
                            const bool live = col < V;
                            const float bA = bAl[col], db = dbl[col];
                            const bool okc[4] = {ok[0] && live, ok[1] && live, ok[2] && live, ok[3] && live};
                            const float m[4] = {x[0], x[1], x[2], x[3]};
                            if (grp) group_x(b1, m, bA, db, col);
                            else ais_draw_v<GAUSS>(kv, grow0, col, b1, bA, db, m, okc, v, s);
                            if constexpr (CLAMP && !GROUPS) ais_clamp(ob, held, v, s);
                            if constexpr (!GROUPS) put_v(v, s, col, TRACE && a.trace_v ? a.trace_v + (int64_t)k * M * ldv : nullptr);
                        });
                if constexpr (GROUPS) {                                // (sm_down's closing barrier: PX is complete)
                    group_pick(kv, v, s);
                    if (tid < L.V64) {
                        if constexpr (CLAMP) ais_clamp(ob, held, v, s);
                        put_v(v, s, tid, TRACE && a.trace_v ? a.trace_v + (int64_t)k * M * ldv : nullptr);
                    }
                    SM_SYNC();
                }
                if (tid < SM_ROWS) {
                    s1 = 0.f;
                    for (int t = 0; t < L.tiles_dn; ++t) s1 += redV[tid * 8 + t];
                }
            }
            b0 = b1; b1 = b_next;
        }

        // ---- what the next launch (or the caller) reads: the visible state and log w
        if (a.v_state) {
            for (int i = tid; i < SM_ROWS * (int)ldv; i += SM_NT) {
                const int e = i / (int)ldv, col = i - e * (int)ldv;
                if (row0 + e < M) a.v_state[(int64_t)(row0 + e) * ldv + col] = X[e * L.ldx + col];
            }
        }
        if (tid < SM_ROWS && row0 + tid < M) a.logw[row0 + tid] = lw;
    }
}

bool ais_small_ok(int64_t M, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh)
{
    return small_shape_ok(M, V, H, gauss) && small_ld_ok(V, H, ldv, ldh);
}

hipError_t launch_ais_small(const AisSmallArgs& a, hipStream_t s)
{
    if (!ais_small_ok(a.M, a.V, a.H, a.gauss, a.ldv, a.ldh) || a.k0 < 0 || a.k1 <= a.k0 || a.k1 > a.K || !ais_clamp_ok(a))
        return hipErrorInvalidValue;
    if (!ais_groups_ok(a.groups, a.V, a.gauss)) return hipErrorInvalidValue;
    const SmallLayout L = small_layout(a.V, a.H, a.gauss != 0);
    const bool trace = a.trace_h || a.trace_v;
    const int variant = a.groups.on ? 8 | (a.mask ? 2 : 0) | (trace ? 1 : 0) : (a.mask ? 4 : 0) | (a.gauss ? 2 : 0) | (trace ? 1 : 0);
    void (*const kerns[12])(AisSmallArgs) = {
        ais_small_kernel<false, false, false>, ais_small_kernel<false, true, false>, ais_small_kernel<true, false, false>,
        ais_small_kernel<true, true, false>,   ais_small_kernel<false, false, true>, ais_small_kernel<false, true, true>,
        ais_small_kernel<true, false, true>,   ais_small_kernel<true, true, true>,
        ais_small_kernel<false, false, false, true>, ais_small_kernel<false, true, false, true>,
        ais_small_kernel<false, false, true, true>,  ais_small_kernel<false, true, true, true>};
    // one workgroup per slab up to one per CU of the chip (no partials to sum here: the cap only bounds the W stagings)
    const int nslabs = (a.M + SM_ROWS - 1) / SM_ROWS;
    const dim3 grid(nslabs < 256 ? nslabs : 256), block(SM_NT);
    AisSmallArgs k = a;
    k.L = L;
    return launch_small_variant(kerns, variant, grid, block, L.bytes, s, k);
}

// ----------------------------------------------------------------------------------
// General path: a workgroup of AIS_NT threads owns one four-chain group; a thread walks the columns tid, tid + AIS_NT, ...
// and the four row sums are combined wave by wave in a fixed order.
// ----------------------------------------------------------------------------------
// one wave per mask row (no mask: one row with nothing held): a held column enters the sum as 0.f
__global__ __launch_bounds__(64) void ais_d2_kernel(const float* vbias, const float* base_vbias, const float* mask, int V, int64_t ldv, float* d2)
{
    const float* mrow = mask ? mask + (int64_t)blockIdx.x * ldv : nullptr;
    float t = 0.f;
    for (int i = threadIdx.x; i < V; i += 64) { const float d = mrow && mrow[i] != 0.f ? 0.f : vbias[i] - base_vbias[i]; t += d * d; }
    t = wave_sum(t);
    if (threadIdx.x == 0) d2[blockIdx.x] = t;
}

__global__ __launch_bounds__(AIS_NT) void ais_hidden_kernel(AisStepArgs a)
{
    __shared__ float red[4 * (AIS_NT / 64)];
    const int row0 = (int)blockIdx.x * 4, tid = threadIdx.x;
    const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
    const float b1 = a.betas[a.k], b0 = a.betas[a.k - 1];
    const bool draw = a.k < a.K;
    PhiloxKey key = a.rng;
    key.step = a.rng.step + (uint32_t)(2 * a.k - 1);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int col = tid; col < (int)a.ldh; col += AIS_NT) {
        const bool live = col < a.H;
        bool ok[4];
        float pre[4], h[4], d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ok[e] = live && row0 + e < a.M;
            pre[e] = ok[e] ? a.pre[(int64_t)(row0 + e) * a.ldh + col] : 0.f;
        }
        ais_draw_h(key, grow0, col, b1, b0, draw, pre, ok, h, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += d[e];
            if (row0 + e < a.M) {
                a.h[(int64_t)(row0 + e) * a.ldh + col] = h[e];          // (pad columns: zeros)
                if (a.trace && draw) a.trace[(int64_t)(row0 + e) * a.ldh + col] = h[e];
            }
        }
    }
    rows4_block_sum<AIS_NT>(acc, red);
    if (tid < 4 && row0 + tid < a.M) {
        const float hsum = tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : acc[3];
        const double lw = a.k == 1 ? 0.0 : a.logw[row0 + tid];
        const float d2 = a.gauss ? a.d2[a.mask_rows == 1 ? 0 : (row0 + tid) / a.C] : 0.f;      // the chain's mask row's
        a.logw[row0 + tid] = ais_logw_add(lw, hsum, a.s1[row0 + tid], d2, b1, b0, a.gauss != 0);
    }
}

template <bool GAUSS, bool CLAMP>
__global__ __launch_bounds__(AIS_NT) void ais_visible_kernel(AisStepArgs a)
{
    __shared__ float red[4 * (AIS_NT / 64)];
    const int row0 = (int)blockIdx.x * 4, tid = threadIdx.x;
    const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
    const float beta = a.k == 0 ? 0.0f : a.betas[a.k];
    PhiloxKey key = a.rng;
    key.step = a.rng.step + (uint32_t)(2 * a.k);
    int64_t drow[4];                         // (clamp) where the chain's data row starts in obs (and in a per-row mask)
    if constexpr (CLAMP) {
#pragma unroll
        for (int e = 0; e < 4; ++e) drow[e] = (int64_t)((row0 + e) / a.C) * a.ldv;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int col = tid; col < (int)a.ldv; col += AIS_NT) {
        const bool live = col < a.V;
        const float bA = live ? a.base_vbias[col] : 0.f, db = live ? a.vbias[col] - bA : 0.f;
        bool ok[4], held[4];
        float m[4], v[4], s[4], ob[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ok[e] = live && row0 + e < a.M;
            m[e] = ok[e] && a.k > 0 ? a.pre[(int64_t)(row0 + e) * a.ldv + col] : 0.f;
            if constexpr (CLAMP) {
                held[e] = ok[e] && a.mask[(a.mask_rows == 1 ? 0 : drow[e]) + col] != 0.f;
                ob[e] = held[e] ? a.obs[drow[e] + col] : 0.f;
            }
        }
        ais_draw_v<GAUSS>(key, grow0, col, beta, bA, db, m, ok, v, s);
        if constexpr (CLAMP) ais_clamp(ob, held, v, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += s[e];
            if (row0 + e < a.M) {
                a.v[(int64_t)(row0 + e) * a.ldv + col] = v[e];
                if (a.trace) a.trace[(int64_t)(row0 + e) * a.ldv + col] = v[e];
            }
        }
    }
    rows4_block_sum<AIS_NT>(acc, red);
    if (tid < 4 && row0 + tid < a.M) a.s1[row0 + tid] = tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : acc[3];
}

// ais_visible_kernel<false, false> for a layer with softmax groups: a thread walks UNITS tid, tid + AIS_NT, ... -- the unit map
// of GroupSoftmaxArgs (mdbn_groups.h), with the pad columns V .. ldv - 1 as Bernoulli units behind the span, written as zeros
// like the plain kernel writes them.  A Bernoulli unit is the plain kernel's column; a group is walked three times per chain
// (group_draw: max, Z, means) with x_c formed from a.pre on the fly, its uniform the Philox word of its first column.  With
// n_groups = 0 a unit is a column and every sum has the plain kernel's operands in its order: the same bits.
// CLAMP: a Bernoulli unit is ais_visible_kernel<false, true>'s column; a group is held by the mask entry at its first column, and
// then its columns take obs and add 0.f to s1 (the draw is made and not used).
template <bool CLAMP>
__global__ __launch_bounds__(AIS_NT) void ais_visible_grouped_kernel(AisStepArgs a)
{
    __shared__ float red[4 * (AIS_NT / 64)];
    const int row0 = (int)blockIdx.x * 4, tid = threadIdx.x;
    const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
    const float beta = a.k == 0 ? 0.0f : a.betas[a.k];
    PhiloxKey key = a.rng;
    key.step = a.rng.step + (uint32_t)(2 * a.k);
    const AisGroups& G = a.groups;
    const int units = G.span_lo + G.n_groups + ((int)a.ldv - G.span_hi);
    int64_t drow[4];                         // (clamp) where the chain's data row starts in obs (and in a per-row mask)
    if constexpr (CLAMP) {
#pragma unroll
        for (int e = 0; e < 4; ++e) drow[e] = (int64_t)((row0 + e) / a.C) * a.ldv;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int unit = tid; unit < units; unit += AIS_NT) {
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
            bool ok[4], held[4];
            float m[4], v[4], s[4], ob[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ok[e] = live && row0 + e < a.M;
                m[e] = ok[e] && a.k > 0 ? a.pre[(int64_t)(row0 + e) * a.ldv + col] : 0.f;
                if constexpr (CLAMP) {
                    held[e] = ok[e] && a.mask[(a.mask_rows == 1 ? 0 : drow[e]) + col] != 0.f;
                    ob[e] = held[e] ? a.obs[drow[e] + col] : 0.f;
                }
            }
            ais_draw_v<false>(key, grow0, col, beta, bA, db, m, ok, v, s);
            if constexpr (CLAMP) ais_clamp(ob, held, v, s);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e] += s[e];
                if (row0 + e < a.M) {
                    a.v[(int64_t)(row0 + e) * a.ldv + col] = v[e];
                    if (a.trace) a.trace[(int64_t)(row0 + e) * a.ldv + col] = v[e];
                }
            }
            continue;
        }
        uint32_t w[4];
        philox_rows4(key, 0u, grow0, (uint32_t)c0, w);
        const float* bAp = a.base_vbias + c0;
        const float* bp = a.vbias + c0;
        bool live[4], held[4] = {false, false, false, false};
        int64_t off[4];
        float u[4], se[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            live[e] = row0 + e < a.M;
            off[e] = (int64_t)(row0 + e) * a.ldv + c0;
            u[e] = philox_u01(w[e]);
            if constexpr (CLAMP) held[e] = live[e] && a.mask[(a.mask_rows == 1 ? 0 : drow[e]) + c0] != 0.f;
        }
        const bool has_m = a.k > 0;
        group_draw(K, u,
                   [&](int c, int e) {
                       const float bA = bAp[c];
                       return tempered_pre_v(beta, live[e] && has_m ? a.pre[off[e] + c] : 0.f, bA, bp[c] - bA);
                   },
                   [&](int c, int e, float v) {
                       if (!live[e]) return;
                       float sc = v * (bp[c] - bAp[c]);
                       if constexpr (CLAMP) {
                           v = held[e] ? a.obs[drow[e] + c0 + c] : v;
                           sc = held[e] ? 0.f : sc;
                       }
                       se[e] += sc;
                       a.v[off[e] + c] = v;
                       if (a.trace) a.trace[off[e] + c] = v;
                   });
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += se[e];
    }
    rows4_block_sum<AIS_NT>(acc, red);
    if (tid < 4 && row0 + tid < a.M) a.s1[row0 + tid] = tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : acc[3];
}

hipError_t launch_ais_d2(const AisStepArgs& a, float* d2, hipStream_t s)
{
    if (!ais_clamp_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ais_d2_kernel, dim3(a.mask_rows), dim3(64), 0, s, a.vbias, a.base_vbias, a.mask, a.V, a.ldv, d2);
    return hipGetLastError();
}

hipError_t launch_ais_hidden(const AisStepArgs& a, hipStream_t s)
{
    if (!ais_clamp_ok(a) || a.k < 1 || a.k > a.K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ais_hidden_kernel, dim3((a.M + 3) / 4), dim3(AIS_NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ais_visible(const AisStepArgs& a, hipStream_t s)
{
    if (!ais_clamp_ok(a) || a.k < 0 || a.k >= a.K || !ais_groups_ok(a.groups, a.V, a.gauss)) return hipErrorInvalidValue;
    const dim3 grid((a.M + 3) / 4), block(AIS_NT);
    if (a.groups.on) {
        if (a.mask) hipLaunchKernelGGL(ais_visible_grouped_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(ais_visible_grouped_kernel<false>, grid, block, 0, s, a);
    } else if (a.mask) {
        if (a.gauss) hipLaunchKernelGGL((ais_visible_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ais_visible_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (a.gauss) hipLaunchKernelGGL((ais_visible_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ais_visible_kernel<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace mdbn

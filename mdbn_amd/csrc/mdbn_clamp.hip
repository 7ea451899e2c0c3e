// Clamped Gibbs sampling of a trained RBM / GRBM on gfx950 / MI355X: the chain of gibbs_vhv with part of the visible layer
// held at observed values, and the running means of its conditional expectations -- the posterior of a missing block of
// visibles (a missing modality under the joint layer of a multimodal DBN) given the observed ones.
//
//   on entry v := mask ? obs : v;  step t = 0 .. n_steps - 1:
//     h_mean = sigmoid(v W + c),                h_sample = (U(step + 2t) < h_mean)
//     RBM : v_mean = sigmoid(h_sample W^T + b), v_new = (U(step + 2t + 1) < v_mean)
//     GRBM: v_mean = h_mean W^T + b,            v_new = v_mean [+ N(0, 1) from step + 2t + 1]      (gauss = 1: the reference's chain)
//           v_mean = h_sample W^T + b,          v_new = v_mean + N(0, 1)                          (gauss = 2: a Gibbs sampler)
//     v_mean := mask ? obs : v_mean;  v := mask ? obs : v_new
//     t >= burn_in:  v_acc += v_mean;  h_acc += h_mean                       (float32, in step order)
// Random draws: draw index 0, the usual (column, global row >> 2) addressing of mdbn_gibbs_chain -- so a run cut into several
// launches, the one-launch path and the general path all meet the same uniforms.
//
// clamp_small_kernel (LDS-resident layers): the shape of ais_small_kernel -- W staged once into the workgroup's LDS, a
// workgroup owns four-row slabs (one Philox block) and runs every step of the launch on the exact-f32 4x4x1 MFMA passes of
// mdbn_small_passes.h.  Both passes hand column `tid` to thread `tid` (propup: one column per thread of the epilogue,
// H64 <= 512; propdown: wave w owns tile w, tiles_dn <= 8), so a thread keeps its column's observed values, mask bits, last
// means and both accumulators in REGISTERS for the whole launch: LDS holds only W and the two 4-row operands, and global
// memory is touched at the two ends of a launch and by the optional taps.
// clamp_step_kernel (any shape): the element-wise clamp + accumulate after the library's propup / propdown passes.
//
// Softmax groups (mdbn_gibbs_clamped_grouped): a Bernoulli layer that holds a span of one-hot groups between Bernoulli columns.
// A free group's draw is one category of softmax_c((h_sample W^T)_c + b_c) -- the group draw of mdbn_sampler_kit.h, ONE uniform
// per (row, group): the Philox word of the group's first column -- and its v_mean the softmax; a group is held or free as a
// WHOLE, by the mask entry at its first column.  clamp_small_kernel<false, ., GROUPS = true>: a thread owns one column, the
// group's pre-activations, exponentials and means travel through the layout's unused X0 / Xb as [column][4] (three barriers per
// step more).  clamp_step_grouped_kernel (any shape): after the propup pass and a LINEAR propdown pass a thread owns a 4-row
// block of one unit and draws, clamps, accumulates and taps in one launch.  n_groups = 0: the plain chain bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_device.h"
#include "mdbn_small.h"
#include "mdbn_small_passes.h"
#include "mdbn_sampler_kit.h"
#include "mdbn_clamp.h"

namespace mdbn {

template <bool GAUSS, bool TRACE, bool GROUPS = false>
__global__ __launch_bounds__(SM_NT) void clamp_small_kernel(ClampSmallArgs a)
{
    static_assert(!GROUPS || !GAUSS, "softmax groups: a Bernoulli layer");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const SmallLayout& L = a.L;
    lds_f* const lds = (lds_f*)sm;
    lds_f* const Wl = lds + L.oW;
    lds_f* const X = lds + L.oXa;           // [4][ldx] visible state (after the clamp)
    lds_f* const PX = lds + L.oX0;          // (groups) [V64][4] pre-activations x_c of the group columns, then their means
    lds_f* const EX = lds + L.oXb;          // (groups) [V64][4] e_c = exp(x_c - max): the Bernoulli layout's third row buffer
    lds_f* const Hs = lds + L.oHs;          // [4][ldhs] what propdown reads: h_sample (RBM) | h_mean (GRBM)
    lds_f* const part = lds + L.oPart;
    lds_f* const hbl = lds + L.oHb;
    lds_f* const vbl = lds + L.oVb;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int V = a.V, H = a.H, B = a.B;
    const int64_t ldv = a.ldv, ldh = a.ldh;
    const int nslabs = (B + SM_ROWS - 1) / SM_ROWS;
    const bool feed_sample = !GAUSS || a.gauss == 2;        // what goes down: the hidden sample, or (the reference's GRBM chain) the mean
    const bool noisy = GAUSS && (a.add_noise || a.gauss == 2);

    // ---- the LDS image: W, the biases, zeroed row buffers
    sm_stage_w(Wl, L, a.W, V, ldh, tid);
    sm_stage_bias(hbl, a.hbias, L.H64, H, tid);
    sm_stage_bias(vbl, a.vbias, L.V64, V, tid);
    sm_zero_rows(X, L.ldx, tid);
    sm_zero_rows(Hs, L.ldhs, tid);
    SM_SYNC();

    const bool vthread = tid < L.V64, hthread = tid < L.H64;      // this thread owns visible / hidden column `tid`
    const bool vlive = tid < V, hlive = tid < H;
    const float hb = hthread ? hbl[tid] : 0.f, vb = vthread ? vbl[tid] : 0.f;
    // ---- (groups) this thread's column belongs to the group [c0, c1) for the whole launch; c1 = c0: a Bernoulli column.  The
    // walk of ais_small_kernel<., ., ., GROUPS>, restated (mdbn_ais.hip keeps its own: its lambdas carry the tempered family
    // and the s1 share): the last g with group_start[g] <= tid; the caller checked its host copy, the device copy is clamped
    // to the span all the same, and a walk never leaves [c0, c1)
    int c0 = 0, c1 = 0;
    if constexpr (GROUPS) {
        const ClampGroups& G = a.groups;
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
    const int mcol = grp ? c0 : tid;        // where this column's mask entry is read: a group is held or free as a whole

    for (int slab = blockIdx.x; slab < nslabs; slab += gridDim.x) {
        const int row0 = slab * SM_ROWS;
        const uint64_t grow0 = a.rng.row_offset + (uint64_t)row0;
        bool ok[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ok[e] = row0 + e < B;
        if (slab != (int)blockIdx.x) SM_SYNC();                        // (the previous slab's last readers are done)

        // ---- the slab's state, in the registers of the column's thread
        float vcur[4] = {0.f, 0.f, 0.f, 0.f}, vm[4] = {0.f, 0.f, 0.f, 0.f}, vacc[4] = {0.f, 0.f, 0.f, 0.f};
        float ob[4] = {0.f, 0.f, 0.f, 0.f};
        bool held[4] = {false, false, false, false};
        float hm[4] = {0.f, 0.f, 0.f, 0.f}, hs[4] = {0.f, 0.f, 0.f, 0.f}, hacc[4] = {0.f, 0.f, 0.f, 0.f};
        if (vthread) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (ok[e] && vlive) {
                    const int64_t off = (int64_t)(row0 + e) * ldv + tid;
                    ob[e] = a.obs[off];
                    held[e] = a.mask[(a.mask_rows == 1 ? 0 : off - tid) + (GROUPS ? mcol : tid)] != 0.f;
                    const float x = a.v[off];
                    vcur[e] = held[e] ? ob[e] : x;
                    if (a.t0 > 0) vacc[e] = a.acc_v[off];
                }
                X[e * L.ldx + tid] = vcur[e];
            }
        }
        if (hthread && hlive && a.t0 > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ok[e]) hacc[e] = a.acc_h[(int64_t)(row0 + e) * ldh + tid];
        }
        SM_SYNC();

        for (int t = a.t0; t < a.t1; ++t) {
            const bool acc = t >= a.burn_in;
            PhiloxKey kh = a.rng, kv = a.rng;
            kh.step = a.rng.step + (uint32_t)(2 * t);
            kv.step = a.rng.step + (uint32_t)(2 * t + 1);
            sm_up(X, Wl, L, part, wave, lane, [] {},
                  [&](const sf32x4& x, int col) {                      // col == tid
                      uint32_t w[4];
                      philox_rows4(kh, 0u, grow0, (uint32_t)col, w);
#pragma unroll
                      for (int e = 0; e < 4; ++e) {
                          const bool live = ok[e] && hlive;
                          hm[e] = live ? sigmoidf_(x[e] + hb) : 0.f;
                          hs[e] = live && philox_u01(w[e]) < hm[e] ? 1.0f : 0.0f;
                          Hs[e * L.ldhs + col] = feed_sample ? hs[e] : hm[e];
                          if (acc) hacc[e] += hm[e];
                      }
                      if (TRACE && a.trace_h && col < (int)ldh) {
#pragma unroll
                          for (int e = 0; e < 4; ++e)
                              if (ok[e]) a.trace_h[((int64_t)t * B + row0 + e) * ldh + col] = hs[e];
                      }
                  });
            sm_down(Hs, Wl, L, wave, lane,
                    [&](const sf32x4& x, int col) {                    // col == tid
                        if constexpr (GROUPS) {
                            if (grp) {                                 // the four pre-activations into PX; the draw follows below
                                *(lds_f4*)(PX + 4 * col) = sf32x4{x[0] + vb, x[1] + vb, x[2] + vb, x[3] + vb};
                                return;
                            }
                        }
                        uint32_t wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
                        if (!GAUSS || noisy) philox_rows4(kv, 0u, grow0, (uint32_t)col, wa);
                        if (noisy) philox_rows4(kv, MDBN_NORMAL_BIT, grow0, (uint32_t)col, wb);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool live = ok[e] && vlive;
                            const float pre = x[e] + vb;
                            float m, s;
                            if (GAUSS) {
                                m = pre;
                                s = m;
                                if (noisy) s = m + box_muller(philox_u01(wa[e]), philox_u01(wb[e]));
                            } else {
                                m = sigmoidf_(pre);
                                s = philox_u01(wa[e]) < m ? 1.0f : 0.0f;
                            }
                            vm[e] = !live ? 0.f : held[e] ? ob[e] : m;
                            vcur[e] = !live ? 0.f : held[e] ? ob[e] : s;
                            X[e * L.ldx + col] = vcur[e];
                            if (acc) vacc[e] += vm[e];
                        }
                        if (TRACE && a.trace_v && col < (int)ldv) {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (ok[e]) a.trace_v[((int64_t)t * B + row0 + e) * ldv + col] = vcur[e];
                        }
                    });
            // (groups) the draw of the group columns, every thread of the workgroup, after sm_down's closing barrier (PX is
            // complete): e_c into EX -- ONE exponential per (row, column) --, barrier, Z and the column's mean over x_c in PX,
            // barrier, the running sum of the means up to the thread's own column and its 0 / 1 entry (mdbn_sampler_kit.h: the
            // group draw).  One uniform per (row, group): the Philox word of the group's first column.  Then the clamp and what
            // the Bernoulli columns did in the epilogue, and a barrier before the next sm_up reads X.
            if constexpr (GROUPS) {
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
                    philox_rows4(kv, 0u, grow0, (uint32_t)c0, w);
                    sf32x4 before = {0.f, 0.f, 0.f, 0.f};
                    for (int c = c0; c < tid; ++c) before += *(const lds_f4*)(PX + 4 * c);
                    const sf32x4 me = *(const lds_f4*)(PX + 4 * tid);
                    const sf32x4 upto = before + me;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s = group_entry(philox_u01(w[e]), before[e], upto[e], tid == c1 - 1);
                        vm[e] = !ok[e] ? 0.f : held[e] ? ob[e] : me[e];
                        vcur[e] = !ok[e] ? 0.f : held[e] ? ob[e] : s;
                        X[e * L.ldx + tid] = vcur[e];
                        if (acc) vacc[e] += vm[e];
                    }
                    if (TRACE && a.trace_v) {                          // (tid < span_hi <= V <= ldv)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (ok[e]) a.trace_v[((int64_t)t * B + row0 + e) * ldv + tid] = vcur[e];
                    }
                }
                SM_SYNC();
            }
        }

        // ---- what the next launch (or the caller) reads
        const bool last = a.t1 == a.n_steps;
        const float n_avg = (float)(a.n_steps - a.burn_in);
        if (vthread && tid < (int)ldv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!ok[e]) continue;
                const int64_t off = (int64_t)(row0 + e) * ldv + tid;
                a.v[off] = vcur[e];
                a.v_mean[off] = vm[e];
                if (!last) a.acc_v[off] = vacc[e];
                else if (a.v_avg) a.v_avg[off] = vacc[e] / n_avg;
            }
        }
        if (hthread && tid < (int)ldh) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!ok[e]) continue;
                const int64_t off = (int64_t)(row0 + e) * ldh + tid;
                a.h_mean[off] = hm[e];
                a.h_sample[off] = hs[e];
                if (!last) a.acc_h[off] = hacc[e];
                else if (a.h_avg) a.h_avg[off] = hacc[e] / n_avg;
            }
        }
    }
}

namespace {

// what a launcher asks of the groups: none, or a Bernoulli layer whose span lies inside the row (the rule of launch_group_softmax)
bool clamp_groups_ok(const ClampGroups& g, int V, int gauss)
{
    if (!g.on) return g.n_groups == 0;
    return !gauss && g.n_groups >= 0 && (g.n_groups == 0 || g.group_start) && g.span_lo >= 0 && g.span_lo <= g.span_hi &&
           g.span_hi <= V && (g.n_groups == 0) == (g.span_lo == g.span_hi) && g.n_groups <= g.span_hi - g.span_lo;
}

}  // namespace

bool clamp_small_ok(int64_t B, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh)
{
    return small_shape_ok(B, V, H, gauss) && small_ld_ok(V, H, ldv, ldh);
}

hipError_t launch_clamp_small(const ClampSmallArgs& a, hipStream_t s)
{
    if (!clamp_groups_ok(a.groups, a.V, a.gauss)) return hipErrorInvalidValue;
    if (!clamp_small_ok(a.B, a.V, a.H, a.gauss, a.ldv, a.ldh) || a.t0 < 0 || a.t1 <= a.t0 || a.t1 > a.n_steps ||
        a.burn_in < 0 || a.burn_in >= a.n_steps || (a.mask_rows != 1 && a.mask_rows != a.B))
        return hipErrorInvalidValue;
    const SmallLayout L = small_layout(a.V, a.H, a.gauss != 0);
    const bool trace = a.trace_h || a.trace_v;
    const int variant = a.groups.on ? 4 | (trace ? 1 : 0) : (a.gauss ? 2 : 0) | (trace ? 1 : 0);
    void (*const kerns[6])(ClampSmallArgs) = {clamp_small_kernel<false, false>, clamp_small_kernel<false, true>, clamp_small_kernel<true, false>,
                                              clamp_small_kernel<true, true>, clamp_small_kernel<false, false, true>,
                                              clamp_small_kernel<false, true, true>};
    // one workgroup per slab (small layers leave room for several on a CU); beyond 1024 slabs a workgroup loops.
    // The LDS request is small_layout's whole (the CD step's) so that the passes are shared unchanged: of it this kernel uses W,
    // Xa, Hs, the chunk partials and the two bias rows; X0, Xb, M0, Mn, the three column-sum rows and U lie unused (with groups
    // X0 and Xb hold the group columns' pre-activations / means and exponentials, [column][4]: 4 V64 <= 4 ldx floats each).
    const int nslabs = (a.B + SM_ROWS - 1) / SM_ROWS;
    const dim3 grid(nslabs < 1024 ? nslabs : 1024), block(SM_NT);
    ClampSmallArgs k = a;
    k.L = L;
    return launch_small_variant(kerns, variant, grid, block, L.bytes, s, k);
}

// ----------------------------------------------------------------------------------
// General path: one thread per element of the [B][ldv] and of the [B][ldh] matrices (grid-stride)
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(CLAMP_NT) void clamp_step_kernel(ClampStepArgs a)
{
    const int64_t nv = (int64_t)a.B * a.ldv, nh = (int64_t)a.B * a.ldh;
    const int64_t stride = (int64_t)gridDim.x * CLAMP_NT;
    for (int64_t i = (int64_t)blockIdx.x * CLAMP_NT + threadIdx.x; i < nv; i += stride) {
        const int64_t row = i / a.ldv;
        const int col = (int)(i - row * a.ldv);
        const bool held = col < a.V && a.mask[(a.mask_rows == 1 ? 0 : row * a.ldv) + col] != 0.f;
        const float o = held ? a.obs[i] : 0.f;
        const float s = held ? o : a.v_new[i];
        a.v[i] = s;
        if (a.entry) continue;
        const float m = held ? o : a.v_mean[i];
        a.v_mean[i] = m;
        if (a.accumulate) {
            const float t = a.acc_v[i] + m;
            a.acc_v[i] = t;
            if (a.last && a.v_avg) a.v_avg[i] = t / a.n_avg;
        }
        if (a.trace_v) a.trace_v[i] = s;
    }
    if (a.entry) return;
    for (int64_t i = (int64_t)blockIdx.x * CLAMP_NT + threadIdx.x; i < nh; i += stride) {
        if (a.accumulate) {
            const float t = a.acc_h[i] + a.h_mean[i];
            a.acc_h[i] = t;
            if (a.last && a.h_avg) a.h_avg[i] = t / a.n_avg;
        }
        if (a.trace_h) a.trace_h[i] = a.h_sample[i];
    }
}

hipError_t launch_clamp_step(const ClampStepArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.H < 1 || (a.mask_rows != 1 && a.mask_rows != a.B)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)a.B * (a.ldv > a.ldh ? a.ldv : a.ldh);
    const int64_t blocks = (n + CLAMP_NT - 1) / CLAMP_NT;
    hipLaunchKernelGGL(clamp_step_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(CLAMP_NT), 0, s, a);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------
// General path of a layer with softmax groups: the visible draw, the clamp, the accumulators and the taps of a step in ONE
// kernel (group_softmax_kernel and clamp_step_kernel as two launches would cost a launch more per step).  The grid of
// group_softmax_kernel: a thread owns a 4-row block -- the shape one Philox block serves -- of one unit of the unit map of
// GroupSoftmaxArgs, with the pad columns V .. ldv - 1 as units behind the span, written as zeros.  On entry v_mean holds the
// linear pre-activations h_sample W^T + vbias; a thread replaces its unit's in place (it reads an entry before it writes it).
//   Bernoulli column: mean = sigmoidf_(x), sample = u < mean with the column's own uniform -- the activation epilogue's draw.
//   group:            group_draw (mdbn_sampler_kit.h), four rows abreast, the uniform of the group's FIRST column; held or free
//                     as a whole by the mask entry at that column.
// The hidden half is clamp_step_kernel's, grid-stride.  `entry`: only v := held ? obs : v.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(CLAMP_NT) void clamp_step_grouped_kernel(ClampStepGroupedArgs ga, int unit_blocks, int units)
{
    const ClampStepArgs& a = ga.c;
    const ClampGroups& G = ga.groups;
    const int bx = (int)blockIdx.x % unit_blocks, by = (int)blockIdx.x / unit_blocks;
    const int unit = bx * CLAMP_NT + (int)threadIdx.x;
    const int r0 = 4 * by;
    if (unit < units) {
        int c0, K = 0;                                   // first column; K = 0: a Bernoulli (or pad) column
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
        const bool vlive = c0 < a.V;
        bool ok[4], held[4];
        int64_t off[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ok[e] = r0 + e < a.B;
            off[e] = (int64_t)(r0 + e) * a.ldv + c0;
            held[e] = ok[e] && vlive && a.mask[(a.mask_rows == 1 ? 0 : off[e] - c0) + c0] != 0.f;
        }
        const int width = K == 0 ? 1 : K;
        // one (row, column) of the unit after its draw: the clamp, the state, the accumulator, the tap
        auto put = [&](int c, int e, float s, float m) {
            if (!ok[e]) return;
            const int64_t i = off[e] + c;
            const float o = held[e] ? a.obs[i] : 0.f;
            s = !vlive ? 0.f : held[e] ? o : s;
            m = !vlive ? 0.f : held[e] ? o : m;
            a.v[i] = s;
            a.v_mean[i] = m;
            if (a.accumulate) {
                const float t = a.acc_v[i] + m;
                a.acc_v[i] = t;
                if (a.last && a.v_avg) a.v_avg[i] = t / a.n_avg;
            }
            if (a.trace_v) a.trace_v[i] = s;
        };
        if (a.entry) {
            for (int c = 0; c < width; ++c) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!ok[e]) continue;
                    const int64_t i = off[e] + c;
                    a.v[i] = !vlive ? 0.f : held[e] ? a.obs[i] : a.v[i];
                }
            }
        } else {
            uint32_t w[4];
            philox_rows4(ga.rng, 0u, ga.rng.row_offset + (uint64_t)r0, (uint32_t)c0, w);
            float u[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = philox_u01(w[e]);
            if (K == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float m = sigmoidf_(ok[e] && vlive ? a.v_mean[off[e]] : 0.f);
                    put(0, e, u[e] < m ? 1.0f : 0.0f, m);
                }
            } else {
                group_draw_mean(K, u, [&](int c, int e) { return ok[e] ? a.v_mean[off[e] + c] : 0.f; }, put);
            }
        }
    }
    if (a.entry) return;
    const int64_t nh = (int64_t)a.B * a.ldh;
    const int64_t stride = (int64_t)gridDim.x * CLAMP_NT;
    for (int64_t i = (int64_t)blockIdx.x * CLAMP_NT + threadIdx.x; i < nh; i += stride) {
        if (a.accumulate) {
            const float t = a.acc_h[i] + a.h_mean[i];
            a.acc_h[i] = t;
            if (a.last && a.h_avg) a.h_avg[i] = t / a.n_avg;
        }
        if (a.trace_h) a.trace_h[i] = a.h_sample[i];
    }
}

hipError_t launch_clamp_step_grouped(const ClampStepGroupedArgs& ga, hipStream_t s)
{
    const ClampStepArgs& a = ga.c;
    const ClampGroups& G = ga.groups;
    if (a.B < 1 || a.V < 1 || a.H < 1 || a.ldv < a.V || (a.mask_rows != 1 && a.mask_rows != a.B) || !G.on ||
        !clamp_groups_ok(G, a.V, 0))
        return hipErrorInvalidValue;
    const int units = G.span_lo + G.n_groups + ((int)a.ldv - G.span_hi);
    const int unit_blocks = (units + CLAMP_NT - 1) / CLAMP_NT;
    const int64_t blocks = (int64_t)unit_blocks * ((a.B + 3) / 4);
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clamp_step_grouped_kernel, dim3((unsigned)blocks), dim3(CLAMP_NT), 0, s, ga, unit_blocks, units);
    return hipGetLastError();
}

}  // namespace mdbn

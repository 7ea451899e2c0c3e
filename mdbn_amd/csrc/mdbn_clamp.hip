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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_device.h"
#include "mdbn_small.h"
#include "mdbn_small_passes.h"
#include "mdbn_sampler_kit.h"
#include "mdbn_clamp.h"

namespace mdbn {

template <bool GAUSS, bool TRACE>
__global__ __launch_bounds__(SM_NT) void clamp_small_kernel(ClampSmallArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const SmallLayout& L = a.L;
    lds_f* const lds = (lds_f*)sm;
    lds_f* const Wl = lds + L.oW;
    lds_f* const X = lds + L.oXa;           // [4][ldx] visible state (after the clamp)
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
                    held[e] = a.mask[(a.mask_rows == 1 ? 0 : off - tid) + tid] != 0.f;
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

bool clamp_small_ok(int64_t B, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh)
{
    return small_shape_ok(B, V, H, gauss) && small_ld_ok(V, H, ldv, ldh);
}

hipError_t launch_clamp_small(const ClampSmallArgs& a, hipStream_t s)
{
    if (!clamp_small_ok(a.B, a.V, a.H, a.gauss, a.ldv, a.ldh) || a.t0 < 0 || a.t1 <= a.t0 || a.t1 > a.n_steps ||
        a.burn_in < 0 || a.burn_in >= a.n_steps || (a.mask_rows != 1 && a.mask_rows != a.B))
        return hipErrorInvalidValue;
    const SmallLayout L = small_layout(a.V, a.H, a.gauss != 0);
    const bool trace = a.trace_h || a.trace_v;
    const int variant = (a.gauss ? 2 : 0) | (trace ? 1 : 0);
    void (*const kerns[4])(ClampSmallArgs) = {clamp_small_kernel<false, false>, clamp_small_kernel<false, true>, clamp_small_kernel<true, false>,
                                              clamp_small_kernel<true, true>};
    // one workgroup per slab (small layers leave room for several on a CU); beyond 1024 slabs a workgroup loops.
    // The LDS request is small_layout's whole (the CD step's) so that the passes are shared unchanged: of it this kernel uses W,
    // Xa, Hs, the chunk partials and the two bias rows; X0, Xb, M0, Mn, the three column-sum rows and U lie unused.
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

}  // namespace mdbn

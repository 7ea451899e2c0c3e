// Clamped annealed importance sampling of a trained RBM / GRBM (mdbn_cais.hip): arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_small.h"
#include "mdbn_ais.h"

namespace mdbn {

// One-launch path (LDS-resident layers, ais_small_ok): temperatures k0 + 1 .. k1 of chains 0 .. M - 1, M = N C; chain m is
// clamped to data row m / C.  Everything AisSmallArgs holds, with the same meaning, and the clamp.
struct CaisSmallArgs {
    int M, V, H, gauss;
    int64_t ldv, ldh;                                // leading dimensions of obs / mask / v_state / the traces; W is [V][ldh]
    const float* W; const float* hbias; const float* vbias; const float* base_vbias;
    const float* betas;                              // [K + 1] device
    int K, k0, k1;                                   // the whole schedule's length; this launch's temperatures (k0, k1]
    PhiloxKey rng;                                   // .step = the run's first step; .draw unused (always 0)
    SmallLayout L;                                   // LDS layout (small_layout; filled in by launch_cais_small)
    const float* obs; const float* mask;             // [M / C][ldv]; [mask_rows][ldv], entries 0 / 1 (1 = held at obs)
    int mask_rows, C;                                // 1 (one row for every data row) | M / C; chains per data row
    float* v_state;                                  // [M][ldv]: k0 > 0: v_{k0 + 1} on entry; v_{min(k1 + 1, K)} on return
    double* logw;                                    // [M]: k0 > 0: log w after temperature k0 on entry; after k1 on return
    float* trace_h; float* trace_v;                  // [K - 1][M][ldh], [K][M][ldv] or NULL
};

// General path, per temperature k: AisStepArgs and the clamp.  d2 holds one sum per mask row (cais_d2_kernel).
struct CaisStepArgs {
    int M, V, H, gauss, k, K;
    int64_t ldv, ldh;
    const float* betas;
    const float* vbias; const float* base_vbias;
    PhiloxKey rng;                                   // .step = the run's first step
    const float* obs; const float* mask;             // [M / C][ldv]; [mask_rows][ldv]
    int mask_rows, C;
    float* pre;                                      // [M][ldh] propup output / [M][ldv] propdown output (m)
    float* h;                                        // [M][ldh] hidden sample
    float* v;                                        // [M][ldv] visible state (after the clamp)
    float* s1;                                       // [M]: sum over the free columns
    const float* d2;                                 // [mask_rows]: sum over the free columns of (b - b_A)^2 (Gaussian)
    double* logw;                                    // [M]
    float* trace;                                    // this temperature's trace slot or NULL
};

hipError_t launch_cais_small(const CaisSmallArgs& a, hipStream_t s);
hipError_t launch_cais_d2(const float* vbias, const float* base_vbias, const float* mask, int mask_rows, int V, int64_t ldv, float* d2,
                          hipStream_t s);
hipError_t launch_cais_hidden(const CaisStepArgs& a, hipStream_t s);
hipError_t launch_cais_visible(const CaisStepArgs& a, hipStream_t s);     // a.k = 0: draws v_1 from the base model (pre unused)

}  // namespace mdbn

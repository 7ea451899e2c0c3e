// Annealed importance sampling of a trained RBM / GRBM, free or with part of the visible layer held at observed values
// (mdbn_ais.hip): arguments and launchers.  The clamp: chain m of the M = N C chains belongs to data row m / C and keeps the
// columns where that row's mask is 1 at obs.  mask == NULL: no clamp (then C = mask_rows = 1 and obs is not read); a mask of
// zeros runs the clamped kernels all the same -- the launchers never look at what a mask holds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_small.h"

namespace mdbn {

constexpr int AIS_CUT = 4096;               // temperatures one launch of the one-launch path runs at most: a launch stays short
                                            // (~3 us per temperature) and the Philox addressing makes the cut invisible
constexpr int AIS_NT = 256;                 // threads of the general path's per-temperature kernels: one wave per chain

// Categorical visible units (mdbn_ais_run_grouped): the unit map of GroupSoftmaxArgs (mdbn_groups.h) -- group g is columns
// group_start[g] .. group_start[g + 1] - 1 of the span [span_lo, span_hi), the columns outside it are Bernoulli units.  `on`
// selects the grouped kernels (n_groups = 0 with `on`: they run with every column a Bernoulli unit and give the plain run
// bit for bit).  span_lo / span_hi come from the caller's checked host copy; what the device copy says is clamped to them.
struct AisGroups {
    const int32_t* group_start;                      // device [n_groups + 1] (not read with n_groups = 0)
    int n_groups, span_lo, span_hi, on;
};

// One-launch path (LDS-resident layers, small_shape_ok): temperatures k0 + 1 .. k1 of chains 0 .. M - 1.
struct AisSmallArgs {
    int M, V, H, gauss;
    int64_t ldv, ldh;                                // leading dimensions of v_state / the traces; W is [V][ldh]
    const float* W; const float* hbias; const float* vbias; const float* base_vbias;
    const float* betas;                              // [K + 1] device
    int K, k0, k1;                                   // the whole schedule's length; this launch's temperatures (k0, k1]
    PhiloxKey rng;                                   // .step = the run's first step; .draw unused (always 0)
    SmallLayout L;                                   // LDS layout (small_layout; filled in by launch_ais_small)
    const float* obs; const float* mask;             // [M / C][ldv]; [mask_rows][ldv], entries 0 / 1 (1 = held at obs) or NULL
    int mask_rows, C;                                // 1 (one row for every data row) | M / C; chains per data row
    float* v_state;                                  // [M][ldv]: k0 > 0: v_{k0 + 1} on entry; v_{min(k1 + 1, K)} on return
    double* logw;                                    // [M]: k0 > 0: log w after temperature k0 on entry; after k1 on return
    float* trace_h; float* trace_v;                  // [K - 1][M][ldh], [K][M][ldv] or NULL
    AisGroups groups;                                // softmax groups of the visible layer (Bernoulli; free or clamped) or {}
};

// General path, per temperature k: pre_h = v_k W + c is in `pre` (the propup GEMM), then
//   hidden : logw += sum_j softplus(b1 pre) - softplus(b0 pre) + bias term (from s1 / d2); h ~ Bernoulli(sigmoid(b1 pre))
//   visible: v_{k+1} from m = h W^T (the propdown GEMM, no bias), then the clamp; s1 = sum_i (v_{k+1} - [gauss] b_A) (b - b_A)
//            over the free columns
struct AisStepArgs {
    int M, V, H, gauss, k, K;
    int64_t ldv, ldh;
    const float* betas;
    const float* vbias; const float* base_vbias;
    PhiloxKey rng;                                   // .step = the run's first step
    const float* obs; const float* mask;             // [M / C][ldv]; [mask_rows][ldv] or NULL
    int mask_rows, C;
    float* pre;                                      // [M][ldh] propup output / [M][ldv] propdown output (m)
    float* h;                                        // [M][ldh] hidden sample
    float* v;                                        // [M][ldv] visible state (after the clamp)
    float* s1;                                       // [M]
    const float* d2;                                 // [mask_rows]: sum over the free columns of (b - b_A)^2 (Gaussian; launch_ais_d2)
    double* logw;                                    // [M]
    float* trace;                                    // this temperature's trace slot or NULL
    AisGroups groups;                                // softmax groups of the visible layer (Bernoulli; free or clamped) or {}
};

bool ais_small_ok(int64_t M, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh);
hipError_t launch_ais_small(const AisSmallArgs& a, hipStream_t s);
hipError_t launch_ais_d2(const AisStepArgs& a, float* d2, hipStream_t s);  // d2[mask_rows] from a.vbias / base_vbias / mask
hipError_t launch_ais_hidden(const AisStepArgs& a, hipStream_t s);
hipError_t launch_ais_visible(const AisStepArgs& a, hipStream_t s);      // a.k = 0: draws v_1 from the base model (pre unused)

}  // namespace mdbn

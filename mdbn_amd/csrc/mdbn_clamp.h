// Clamped Gibbs sampling of a trained RBM / GRBM (mdbn_clamp.hip): arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_small.h"

namespace mdbn {

constexpr int CLAMP_CUT = 2048;             // Gibbs steps one launch of the one-launch path runs at most: a launch stays in the
                                            // millisecond range (a step costs about what an AIS temperature does, mdbn_ais.h);
                                            // the state travels through v and the two accumulators, bit for bit
constexpr int CLAMP_NT = 256;               // threads of the general path's per-step kernel

// Categorical visible units (mdbn_gibbs_clamped_grouped): the unit map of GroupSoftmaxArgs (mdbn_groups.h) -- group g is columns
// group_start[g] .. group_start[g + 1] - 1 of the span [span_lo, span_hi), the columns outside it are Bernoulli units.  `on`
// selects the grouped kernels (n_groups = 0 with `on`: every column a Bernoulli unit, the plain run bit for bit).  span_lo /
// span_hi come from the caller's checked host copy; what the device copy says is clamped to them.  A group is held or free as
// a whole: by the mask entry at its FIRST column.
struct ClampGroups {
    const int32_t* group_start;                      // device [n_groups + 1] (not read with n_groups = 0)
    int n_groups, span_lo, span_hi, on;
};

// One-launch path (LDS-resident layers, small_shape_ok): steps t0 .. t1 - 1 of rows 0 .. B - 1.
struct ClampSmallArgs {
    int B, V, H, gauss, add_noise;                   // gauss: 0 | 1 | 2 as mdbn_gibbs_clamped (2: the hidden SAMPLE goes down, noise always)
    int64_t ldv, ldh;                                // leading dimensions of the [., V] / [., H] matrices; W is [V][ldh]
    const float* W; const float* hbias; const float* vbias;
    float* v;                                        // [B][ldv] the chain's visible state (in and out)
    const float* obs; const float* mask;             // [B][ldv]; [mask_rows][ldv], entries 0 / 1 (1 = held at obs)
    int mask_rows;                                   // 1 (one row for the whole batch) | B
    int n_steps, burn_in, t0, t1;                    // the whole run; this launch's steps [t0, t1)
    PhiloxKey rng;                                   // .step = the run's first step; .draw unused (always 0)
    SmallLayout L;                                   // LDS layout (small_layout; filled in by launch_clamp_small)
    float* h_mean; float* h_sample; float* v_mean;   // step t1 - 1's values
    float* v_avg; float* h_avg;                      // NULL = off; written by the launch with t1 == n_steps
    float* acc_v; float* acc_h;                      // [B][ldv], [B][ldh]: the sums after step t0 - 1 on entry (t0 > 0), after
                                                     // t1 - 1 on return (t1 < n_steps)
    float* trace_h; float* trace_v;                  // [n_steps][B][ldh], [n_steps][B][ldv] or NULL
    ClampGroups groups;                              // .on: clamp_small_kernel<false, ., true> (gauss = 0 only)
};

// General path, after the two propagation passes of a step: the clamp, the accumulators and the taps, element-wise.
struct ClampStepArgs {
    int B, V, H, entry;                              // entry != 0: only v := mask ? obs : v (before the first step)
    int64_t ldv, ldh;
    float* v; float* v_mean;                         // [B][ldv]: the chain state / the mean of the propdown pass; clamped in place
    const float* v_new;                              // where the pass left v_new (v itself, or v_mean: noise-free GRBM)
    const float* obs; const float* mask; int mask_rows;
    const float* h_mean; const float* h_sample;      // [B][ldh]
    int accumulate, last;                            // t >= burn_in; t == n_steps - 1
    float n_avg;                                     // n_steps - burn_in
    float* acc_v; float* acc_h;                      // the running sums (zero before the first accumulated step)
    float* v_avg; float* h_avg;                      // NULL = off; written when `last`
    float* trace_h; float* trace_v;                  // this step's slots or NULL
};

// General path of a layer with softmax groups, after the propup pass and the LINEAR propdown pass of a step (v_mean holds
// h_sample W^T + vbias): the draw, the clamp, the accumulators and the taps in ONE kernel.  A thread owns a 4-row block of one
// unit (a group, a Bernoulli column, or a pad column V .. ldv - 1, which is written as zeros).
struct ClampStepGroupedArgs {
    ClampStepArgs c;                                 // v_new unused: the kernel draws the new state itself
    ClampGroups groups;
    PhiloxKey rng;                                   // the visible draw's key: .step = the run's first step + 2t + 1, draw 0
};

bool clamp_small_ok(int64_t B, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh);
hipError_t launch_clamp_small(const ClampSmallArgs& a, hipStream_t s);
hipError_t launch_clamp_step(const ClampStepArgs& a, hipStream_t s);
hipError_t launch_clamp_step_grouped(const ClampStepGroupedArgs& a, hipStream_t s);

}  // namespace mdbn

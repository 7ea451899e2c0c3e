// Parallel tempering of a trained RBM / GRBM (mdbn_temper.hip): arguments, LDS layout and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_kernels.h"
#include "mdbn_small.h"
#include "mdbn_ais.h"                       // AisGroups: the unit map of a layer with softmax groups

namespace mdbn {

constexpr int PT_CUT = 2048;                // four-row slab passes one launch of the one-launch path runs at most (a slab pass
                                            // costs about what a clamped Gibbs step does: CLAMP_CUT); a launch runs
                                            // max(1, PT_CUT / (R / 4)) sweeps, the state travels through h, the rank map,
                                            // the counts and the two sums, bit for bit
constexpr int PT_NT = 256;                  // threads of the general path's two per-sweep kernels
constexpr int PT_MAX_R = 64;                // temperatures of a ladder on the one-launch path
constexpr int PT_SMALL_MIN_LADDERS = 512;   // ladders from which path = 0 takes the one-launch path (pt_small_preferred)
constexpr int PT_MAX_R_GENERAL = 2048;      // ... on the general path (the ladder's bookkeeping sits in one workgroup's LDS)

// What the one-launch kernel keeps in LDS behind small_layout's buffers (offsets in floats from the start of LDS)
struct PtLayout {
    int oHs, oA;                // [R][ldhs] hidden samples / pre-activations a = v W + c of the ladder's rows
    int oRedH, oRedV;           // [R][8] per-tile partials of the two shares of l(beta_partner) - l(beta_own)
    int oBeta, oRank, oInv;     // [R] betas; rank of a slot; slot of a rank
    int bytes;                  // the whole request (small_layout's included)
};

__host__ __device__ inline PtLayout pt_layout(const SmallLayout& L, int R)
{
    PtLayout P;
    int o = L.bytes / 4;
    auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
    P.oHs = take(R * L.ldhs);
    P.oA = take(R * L.ldhs);
    P.oRedH = take(R * 8); P.oRedV = take(R * 8);
    P.oBeta = take(R); P.oRank = take(R); P.oInv = take(R);
    P.bytes = o * 4;
    return P;
}

// One-launch path: sweeps t0 .. t1 - 1 of M ladders of R replicas (row m R + s = slot s of ladder m).
struct PtSmallArgs {
    int M, R, V, H, gauss;
    int64_t ldv, ldh;                                // leading dimensions of the [., V] / [., H] matrices; W is [V][ldh]
    const float* W; const float* hbias; const float* vbias; const float* base_vbias;
    const float* betas;                              // [R] device
    float* v; float* h;                              // [M R][ldv] (out: the last sweep's draw), [M R][ldh] (in and out)
    int* rank;                                       // [M][R] temperature index of a slot (in and out)
    int* counts;                                     // [M][R - 1] accepted swaps of the run so far (read when t0 > 0)
    float* v_sum; float* h_sum;                      // [M][ldv], [M][ldh] running sums (read when t0 > 0)
    float* v_avg; float* h_avg;                      // [M][ldv], [M][ldh]: written by the launch with t1 == n
    int n, burn_in, t0, t1;                          // the whole run; this launch's sweeps [t0, t1)
    int64_t sweep0;                                  // sweeps the ladders ran before this run: the swap parity continues
    PhiloxKey rng;                                   // .step = the run's first step
    SmallLayout L; PtLayout P;                       // filled in by launch_pt_small
    float* trace_v; float* trace_h; int* trace_swaps;    // [n][M R][ldv], [n][M R][ldh], [n][M][2][R] or NULL
    double* zacc;                                    // [M][R - 1][4] = {m_f, s_f, m_r, s_r} of the works (in and out) or NULL
    double* trace_work;                              // [n][M][R - 1][2] = (d_fwd, d_rev), NaN where not attempted, or NULL
    AisGroups groups;                                // softmax groups of the visible layer (Bernoulli only) or {}
};

// General path, one sweep: pt_visible_kernel (groups.on: pt_visible_grouped_kernel) after the propdown GEMM, pt_swap_hidden_kernel after the propup GEMM.
struct PtStepArgs {
    int M, R, V, H, gauss;
    int64_t ldv, ldh;
    const float* vbias; const float* base_vbias; const float* betas;
    const float* pre;                                // [M R][ldv]: h W^T | [M R][ldh]: v W + c
    float* v; float* h;
    int* rank; int* counts;
    float* s1;                                       // [M R] visible share of l (mdbn_temper.hip)
    float* v_sum; float* h_sum; float* v_avg; float* h_avg;
    int t, accumulate, last; float n_avg;
    int64_t sweep0;
    PhiloxKey rng;
    float* trace_v; float* trace_h; int* trace_swaps;    // this sweep's slots or NULL
    double* zacc;                                    // [M][R - 1][4] (mdbn_temper.hip: the works) or NULL
    double* trace_work;                              // this sweep's [M][R - 1][2] or NULL
    const double* g;                                 // |b - b_A|^2 (launch_pt_gnorm); read when gauss and zacc / trace_work
    AisGroups groups;                                // softmax groups of the visible layer (Bernoulli only) or {}
};

bool pt_small_ok(int64_t M, int64_t R, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh);
bool pt_small_preferred(int64_t M, int64_t R, int64_t V, int64_t H, int gauss, int64_t ldv, int64_t ldh);
int pt_default_cut(int64_t R);
hipError_t launch_pt_small(const PtSmallArgs& a, hipStream_t s);
hipError_t launch_pt_visible(const PtStepArgs& a, hipStream_t s);
hipError_t launch_pt_swap_hidden(const PtStepArgs& a, hipStream_t s);
hipError_t launch_pt_counts(const int* counts, int M, int R, int* accepted, hipStream_t s);
hipError_t launch_pt_gnorm(const float* vbias, const float* base_vbias, int V, double* g, hipStream_t s);

}  // namespace mdbn

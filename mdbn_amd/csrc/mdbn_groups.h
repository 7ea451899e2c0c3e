// Categorical visible units (mdbn_groups.hip): K-ary softmax groups inside a visible layer (Salakhutdinov, Mnih & Hinton
// 2007) -- the conditional p(v | h) of a layer whose visibles are partly one-hot groups, partly Bernoulli units, from the
// pre-activations h W^T + vbias.  Arguments and launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "philox.h"
#include "../../include/mdbn_hip.h"         // MDBN_GROUP_MAX: the largest group (categories of one softmax unit)

namespace mdbn {

constexpr int GROUPS_NT = 256;              // threads of a group_softmax workgroup: 256 units of one 4-row block

// A "unit" is one softmax group or one Bernoulli column; unit u of a row is
//   u < span_lo                     Bernoulli column u
//   u < span_lo + n_groups          group u - span_lo: columns group_start[g] .. group_start[g + 1] - 1
//   else                            Bernoulli column span_hi + (u - span_lo - n_groups)
struct GroupSoftmaxArgs {
    const float* pre;                       // [B][ld] pre-activations (bias included)
    float* mean; float* sample; float* tap; // [B][ld] each, nullable; mean may be `pre` itself (a thread reads a group's
                                            // entry before it writes it)
    const float* v0; float* cost_partials;  // cost target [B][ld] and one partial per workgroup (both or neither)
    const int32_t* group_start;             // device [n_groups + 1] (not read with n_groups = 0)
    int n_groups;
    int span_lo, span_hi;                   // group_start[0], group_start[n_groups] of the caller's checked host copy
                                            // (n_groups = 0: both V); what the device copy says is clamped to them
    int B, V, units;
    int64_t ld;
    PhiloxKey rng;
};

inline int group_units(int V, int span_lo, int span_hi, int n_groups) { return V - (span_hi - span_lo) + n_groups; }
// workgroups (= cost partials) of a launch over `units` units of B rows
inline int64_t group_softmax_blocks(int64_t B, int64_t units) { return ((units + GROUPS_NT - 1) / GROUPS_NT) * ((B + 3) / 4); }

hipError_t launch_group_softmax(const GroupSoftmaxArgs& a, hipStream_t s);

// The hidden-bias statistic of the centred gradient (mdbn_center.hip: s_h' = s_h - rho S'^T mu) formed from the ROWS of the
// step's scratch instead of from S:  S'^T mu = sum_r [d_r ph_r - d_{B+r} nh_r] - (s_v . mu) lam  with  d_r = mu . (x_r - mu)
// over the rows x_r of V2 = [v0; nv].  On one-hot rows mu . x_r is the same for every row up to the offsets' spread, so d_r is
// small and nothing of the size of (mu . mu) s_h is formed and cancelled -- through S that cancellation multiplies the float32
// error of S by sum_i mu_i (256 at 1024 visibles in groups of 4).
struct CenterHiddenArgs {
    const float* V2; const float* P2;       // [2B][ldv], [2B][ldh]: P2's second half holds -nh_mean
    const float* stats;                     // packed [V ldh | ldh | ldv | 4] BEFORE mdbn_center_stats: s_h and s_v are read
    const float* mu; const float* lam;      // [V], [H]
    float* d;                               // workspace [2B + 3]: d_r, then s_v . mu, v_mean . mu, mu . mu
    float* out;                             // [H]: s_h'
    int64_t ldv, ldh;
    int B, V, H;
    float rho;
    // `stats` went through mdbn_sparsity_stats (S += w_scale v_mean t', s_h += b_scale t, t = target - q) before this call:
    // S'^T mu then also holds (w_scale (v_mean . mu) - b_scale (mu . mu)) t, which the rows do not know.  q null: no such transform
    const float* q; const float* v_mean;    // [H], [V] (v_mean null with w_scale = 0)
    float target, w_scale, b_scale;
};
hipError_t launch_center_hidden(const CenterHiddenArgs& a, hipStream_t s);

}  // namespace mdbn

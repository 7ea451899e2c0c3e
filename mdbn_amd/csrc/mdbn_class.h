// Classification RBM (mdbn_class.hip): the exact posterior p(label | everything else) of a one-hot label block inside the
// visible layer and the exact gradient of sum_rows log p(y* | x) (Larochelle & Bengio 2008), from ONE propup of the rows with
// the block set to zero.  With A = hbias + x~ W (that propup's pre-activations), U = the block's K rows of W, d = its K
// visible biases:
//   o[y][j] = A[j] + U[y][j],   a[y] = d[y] + sum_j softplus(o[y][j]),   p(y | x) = softmax_y a[y]
//   r_pos = sigmoid(o[y*][.]),  r_bar = sum_y p(y | x) sigmoid(o[y][.])
//   T[y][.] = sum_rows p(y | x) sigmoid(o[y][.]),   n[y] = sum_rows ([y = y*] - p(y | x))
// Arguments and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mdbn_hip.h"         // MDBN_GROUP_MAX: the widest label block

namespace mdbn {

constexpr int CLASS_NT = 256;               // threads of a class_forward workgroup: lanes run over the hidden units
constexpr int CLASS_NW = CLASS_NT / 64;
constexpr int CLASS_R = 4;                  // rows of one batch of a workgroup (their A values stay in registers in the second pass)
constexpr int CLASS_PREP_ROWS = 32;         // rows of one class_prep chunk (one partial of the visible-bias statistic each)

// x~ and the stacked visible operand of the statistics GEMM, from the rows v0 [B][ldv] (and, hybrid, the chain's nv):
//   posterior         xt                     = x~
//   pure              V2s = [v0; x~]         (xt = rows B.. of V2s)
//   hybrid            V2s = [v0; v0; nv; x~] (xt = rows 3B..), svp[chunk][.] = sum over the chunk's rows of (v0 - nv)
// Pad columns V..ldv-1 of what it writes are set to zero; those of v0 / nv are not read.
struct ClassPrepArgs {
    const float* v0; const float* nv;       // nv null: no hybrid
    float* copy0; float* copy1; float* copy_nv;   // [B][ldv] each, nullable: where v0 (twice) and nv are copied
    float* xt;                              // [B][ldv]
    float* svp;                             // [chunks][ldv], hybrid only
    int B, V, lo, K;
    int64_t ldv;
};
inline int class_prep_chunks(int64_t B) { return (int)((B + CLASS_PREP_ROWS - 1) / CLASS_PREP_ROWS); }
hipError_t launch_class_prep(const ClassPrepArgs& a, hipStream_t s);

// class_forward: a workgroup owns whole rows, R at a time (batch b of workgroup g is rows (g + b G) R ..).
struct ClassForwardArgs {
    const float* A;                         // [B][ldh] pre-activations of x~
    const float* U; const float* d;         // W + lo ldh ([K][ldh]), vbias + lo ([K])
    const float* label;                     // v0 + lo: the rows' label block, row stride ld_label; null: no labels (posterior only)
    int64_t ld_label;
    float* post; int64_t ldk;               // [B][ldk] float32 posterior, nullable
    float* logp;                            // [B] log p(y* | x), nullable (needs label)
    // training mode (rpos != null): the operand rows w r_pos, -w r_bar [B][ldh] each (pad columns zeroed), the copies
    // gen ph -> ph_out, gen (-nh) -> nh_out (ph null: none), and the per-workgroup partials of T, n and -sum logp
    float* rpos; float* rbar;
    const float* ph; const float* nh; float* ph_out; float* nh_out;
    float* Tp;                              // [G][K][ldh]
    float* np;                              // [G][MDBN_GROUP_MAX]
    float* nllp;                            // [G]
    float w, gen;
    int B, H, K, G;
    int R;                                  // rows of a batch, 1 .. CLASS_R
    int64_t ldh;
};
hipError_t launch_class_forward(const ClassForwardArgs& a, hipStream_t s);

// class_patch: sums the partials in ascending workgroup order and applies them to the packed statistics after the GEMM:
//   S[lo + y][0..H) -= w T[y][.];   s_v = gen sum_chunks svp + w n on the block's columns (n = 0 elsewhere);
//   nll_out[0] = -sum logp, and the same into cost_out[0] when that is given (a pure step has no chain and no CD cost).
struct ClassPatchArgs {
    const float* Tp; const float* np; const float* nllp; const float* svp;     // svp null: gen = 0
    float* S; float* s_v; float* nll_out; float* cost_out;
    float w, gen;
    int V, H, K, lo, G, chunks;
    int64_t ldv, ldh;
};
hipError_t launch_class_patch(const ClassPatchArgs& a, hipStream_t s);

}  // namespace mdbn

// What a feature driver of the C ABI (mdbn_comm.hip, mdbn_drv_groups.hip, mdbn_drv_samplers.hip, mdbn_drv_sigma.hip, mdbn_drv_train.hip, mdbn_feeder.hip) may use of
// the core (mdbn_capi.hip): the context record, the error macros, the leading-dimension helpers, the workspace of the
// propagation GEMMs and one affine pass over it, and the two halves of an update rule as a kernel takes them.  The planner, the
// kernel timing and the g_opt_* option names are NOT here: a driver that needs one of them does not compile, and that
// is the point -- it belongs in the core, or the interface needs a decision.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <utility>
#include <vector>
#include "mdbn_kernels.h"

namespace mdbn {
struct UpdownGeom;                         // mdbn_updown.h

namespace capi {

// Tuning knobs of ONE context (mdbn_set_option(ctx, ...) writes ctx->opt; a knob set on one context never changes what
// another context of the process launches).  The option comments sit beside the g_opt_* names of mdbn_capi.hip, which read the
// options of the context whose call is running on this thread (CtxScope).
struct Options {
    int gemm_bk = 0;
    int x6_min_jobs = 48;
    int x6_pw = 4;
    int gemm_cw = 0;
    int update_overlap = 0;
    int fused_epilogue = 1;
    int fused_update = 1;
    int fused_finalize = 1;
    int skinny_gemm = 1;
    int skinny_fused_max_k = 1024;
    int64_t skinny_max_macs = 32ll << 20;
    int stream_x6 = 2;
    int64_t stream_max_macs = (int64_t)1 << 30;
    int stream_mi = 0;
    int stream_ni = 0;
    int gemm_bf16x6 = 3;
    int small_fused = 1;
    int thin_fused = 1;
    int gchain = 0;
    int gemm_planes = 1;
    int planes_mfma = 16;
    int early_w = 1;
    int narrow_tiles = 1;
    int slab_tail = 1;
    int narrow_deep = 1;       // no option name: read once from the process environment when the context is created (mdbn_ctx_create)
    int feed_copy_streams = 1;
    int gather_ahead = 1;
    int bf16_inputs = 0;
    int64_t planes_min_work = (int64_t)1 << 30;
    int comm_cus = 0;
    int bal_blocks = 0;
    int min_splitk = 128;
    int epilogue_cw = 0;
    int epilogue_threads = 0;
    int small_fin_lanes = 0;
};

// Optional HIP-event timing of the GEMM launches (the dominant kernel), used by bench.py to
// quote the roofline from the kernel's own average duration on the stream it runs on.
struct GemmTiming {
    bool enabled = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    // per recorded launch: which GEMM it was and the work it issued (mdbn_kernel_timing_detail)
    struct Meta { int kind; double alg_flop, pipe_flop; };
    std::vector<Meta> meta;
    size_t used = 0;
};

}  // namespace capi
}  // namespace mdbn

// (global: include/mdbn_hip.h declares the type as an opaque C struct)
struct mdbn_ctx {
    int device;
    int num_cu;
    mdbn::capi::Options opt;
    mdbn::capi::GemmTiming timing;                  // mdbn_kernel_timing: per context
    // mdbn_cd_forward -> mdbn_cd_statistics hand-over (host side only): the cost partials the chain's last visible pass left
    int64_t narrow_deep_launches = 0;              // narrow propdown launches that took 64-deep stages (mdbn_narrow_deep_launches)
    int pending_n_cost = -1;
    const void* pending_stats = nullptr;
    void* comm = nullptr;      // ncclComm_t of mdbn_comm_init_rank (RCCL), or NULL
    int comm_ranks = 0;
    // side stream + events for mdbn_cd_train_step (memory-bound update work overlapped with the
    // compute-bound statistics GEMM); created on first use
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // group-chain step (mdbn_gchain.hip): the flag words of its in-launch exchange ([GC_MAX_FLAGS] + one error word; made
    // and zeroed on first use, written by that protocol only) and the sequence number of the next launch's first exchange
    unsigned* gc_flags = nullptr;
    unsigned gc_seq = 1;
};

namespace mdbn {
namespace capi {

// The options / timing records a library call reads are those of the context it was made on: every entry point that takes
// a context opens a CtxScope; context-free entry points (mdbn_workspace_bytes, mdbn_planes_eligible, ...) see the defaults
// of a fresh context.
struct CtxScope {
    const Options* prev_opt; GemmTiming* prev_timing;
    explicit CtxScope(mdbn_ctx* c);
    ~CtxScope();
    CtxScope(const CtxScope&) = delete;
    CtxScope& operator=(const CtxScope&) = delete;
};

// records the message mdbn_last_error returns on this thread; returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_OK(expr)                                                                    \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(MDBN_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                            \
    } while (0)

#define REQUIRE(cond, ...)                                 \
    do {                                                   \
        if (!(cond)) return fail(MDBN_EINVAL, __VA_ARGS__); \
    } while (0)

#define CHECK(expr) do { int _rc = (expr); if (_rc != MDBN_OK) return _rc; } while (0)

constexpr int kTargetJobs = 256;       // one 8-wave tile job per CU (MI355X: 256 CUs)

inline int64_t ru4(int64_t x) { return (x + 3) & ~int64_t(3); }
// Leading-dimension policy (mdbn_padded_ld).  Padding 1-KiB-multiple rows by 64 floats (to spread
// a GEMM slice's rows over the L2 channels) gained ~10% in the isolated GEMM microbenchmark
// (scripts/gemm_ldpad.py) but LOST 2% on the whole CD step (K1 42.3 vs 40.6 us, update 17.0 vs
// 13.5 us, profiles r01e vs r01d), and does nothing for the streaming kernel of the mid-size layers either
// (profiles/r05zc_ldpad.log), so the policy is plain round_up(cols, 4); every entry point
// accepts any ld % 4 == 0, ld >= cols.
inline int64_t padded_ld(int64_t cols) { return ru4(cols); }
inline int64_t ru64(int64_t x) { return (x + 63) & ~int64_t(63); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_mat(const void* p, int64_t ld, int64_t cols, const char* name);
// the table of a layer with softmax groups as the host holds it (mdbn_drv_groups.hip: the rules of mdbn_group_softmax_sample)
// -> the span [lo, hi) the groups cover; n_groups = 0: lo = hi = V
int check_groups(const int32_t* dev, const int32_t* host, int64_t n_groups, int64_t V, int& lo, int& hi);
PhiloxKey make_key(const mdbn_rng& r, uint32_t draw);

// carve-up of the caller's workspace
struct Workspace {
    float* slabs;
    int64_t slab_floats;
    float* cost_partials;
    int64_t cost_floats;
    float* colPpos;   // [row_groups][ldh]  4-row partial column sums of  ph_mean
    float* colPneg;   // [row_groups][ldh]                                -nh_mean
    float* colV;      // [row_groups][ldv]                                 v0 - nv_mean
};

// bytes of the whole carve-up for a (B, V, H) step under the options of the running call (mdbn_workspace_bytes)
int64_t dense_workspace_bytes(int64_t B, int64_t V, int64_t H);
// need_stats: the carve-up of a CD step; else propagation only (a fixed cost region at the end, everything else is slabs)
// ldv / ldh: the leading dimensions of a need_stats call (0: the policy's) -- the column-sum regions lie on them
int carve(void* ws, int64_t bytes, int64_t B, int64_t V, int64_t H, Workspace& out, bool need_stats, int64_t ldv = 0, int64_t ldh = 0);

// One affine map + activation over `rows` rows, chunked so the split-K slabs fit.
//   up   (dir 0): x[rows, V] * W        -> [rows, H]   (bias = hbias)
//   down (dir 1): x[rows, H] * W^T      -> [rows, V]   (bias = vbias)
// The constructors take the operands of a pass; its outputs and options are assigned by name at the call site.
struct Affine {
    const float* x = nullptr; int64_t rows = 0, ldx = 0;
    const float* W = nullptr; int64_t V = 0, H = 0, ldw = 0;
    int dir = 0;
    const float* bias = nullptr;
    float* pre = nullptr; float* mean = nullptr; float* sample = nullptr; int64_t ldo = 0;
    float mean_scale = 1.0f; int gauss = 0;
    const float* target = nullptr; int64_t ld_target = 0;
    bool want_cost = false;
    const mdbn_rng* rng = nullptr; uint32_t draw = 0u;
    float* colsum = nullptr; int colsum_kind = 0;
    // x holds 0/1 samples written by our own epilogues (a Gibbs chain state): exactly representable
    // in bf16, so the bf16x6 kernel needs one piece of it and three products instead of six
    bool x_binary = false;
    // up pass: the output rides on W's leading dimension
    Affine(const float* x, int64_t rows, int64_t ldx, const float* W, int64_t V, int64_t H, int64_t ldw, const float* hbias)
        : x(x), rows(rows), ldx(ldx), W(W), V(V), H(H), ldw(ldw), dir(0), bias(hbias), ldo(ldw) {}
    // down pass
    Affine(const float* x, int64_t rows, int64_t ldx, const float* W, int64_t V, int64_t H, int64_t ldw, const float* vbias,
           int64_t ldo, int gauss) : x(x), rows(rows), ldx(ldx), W(W), V(V), H(H), ldw(ldw), dir(1), bias(vbias), ldo(ldo), gauss(gauss) {}
};

int run_affine(const Affine& a, const Workspace& ws, hipStream_t s, int* n_cost_out);

// the weight half of an update rule as a kernel applies it to its own tile of S (Wp: planes of the new W, or NULL)
void fill_upd(UpdEpi& e, const mdbn_update_args& u, int64_t V, int64_t ldh, unsigned short* Wp);
// ... and its bias / monitoring-cost half (H: the live hidden width)
void fill_bias_upd(BiasUpd& b, const mdbn_update_args& u, int64_t H);

// The delta rules of up-down fine-tuning (mdbn_drv_train.hip), as far as the grouped generative rule (mdbn_drv_groups.hip)
// shares them.  Workspace of a delta-rule step, in floats (every piece a multiple of 64 floats: 16-byte aligned):
struct UpdownWs {
    int64_t V2, P2, pre, mean, stats, junk, partials, inner;
    int64_t total() const { return V2 + P2 + pre + mean + stats + junk + partials + inner; }
};
int updown_check_shape(const mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path);
// the rule's own arguments (`gen`: the visible half is updated, else the hidden)
int updown_check_update(const mdbn_update_args* u, bool gen);
// the carve-up of the generative half: fused = the cost partials of ug.G workgroups only, else the composed path's pieces
int updown_gen_ws(bool fused, const UpdownGeom& ug, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, UpdownWs& w);
float* updown_take(float*& p, int64_t floats);

}  // namespace capi
}  // namespace mdbn

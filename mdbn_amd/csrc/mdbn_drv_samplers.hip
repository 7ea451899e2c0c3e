// C-ABI drivers of the samplers and of the variational bound (declared in include/mdbn_hip.h): annealed importance sampling
// (mdbn_ais.hip), clamped Gibbs sampling (mdbn_clamp.hip), parallel tempering and log Z (mdbn_temper.hip), the per-row
// log-likelihood and the replica draws of the bound (mdbn_bound.hip).  Of the core they use what mdbn_capi_internal.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include "mdbn_capi_internal.h"
#include "mdbn_ais.h"
#include "mdbn_clamp.h"
#include "mdbn_temper.h"
#include "mdbn_bound.h"

using namespace mdbn;
using namespace mdbn::capi;

extern "C" {

// ---------------------------------------------------------------------------------- what the three sampler drivers share
namespace {

// Scratch of the propagation GEMMs of a general path (carve: slabs + a fixed cost region).  Any size serves (a pass is chunked
// until its split-K slabs fit); what the plans of `rows` rows ask for is not monotone in the rows (fewer rows: more split-K), so
// with cover_fewer_rows the answer is the largest over `rows` and the whole 32-row tilings below it -- a buffer sized for
// `rows` rows serves any fewer
int64_t gemm_scratch_bytes(int64_t rows, int64_t V, int64_t H, bool cover_fewer_rows)
{
    int64_t g = dense_workspace_bytes(rows, V, H);
    if (cover_fewer_rows) {
        const int64_t step = std::max<int64_t>(32, ((rows >> 12) + 31) & ~int64_t(31));
        for (int64_t m = step; m < rows; m += step) g = std::max(g, dense_workspace_bytes(m, V, H));
    }
    return g + 4 * ((int64_t)(1 << 16) + 4096);
}

// The path a *_workspace_bytes call sizes for.  One buffer serves a layer whatever its visible type, so path 1 needs the layer
// to fit for either type, and path 0 sizes for the one-launch path only where a run would take it for both.  -1: path 1 was
// asked for and the layer fits for neither.
int sizing_path(int path, bool fits_either, bool taken_both)
{
    if (path == 1) return fits_either ? 1 : -1;
    return path == 0 && taken_both ? 1 : 2;
}

// The path a run takes: path = 0 chooses by shape
int run_path(int path, bool one_launch) { return path == 0 ? (one_launch ? 1 : 2) : path; }

// Two groups of argument rules the three run entry points share; an entry point checks its own rules before, between and after
// them (the API tests assert which error a bad call reports, and that it comes without a device: the order stays).
int sampler_workspace_rules(int64_t workspace_bytes, int64_t need, const char* sizer, const mdbn_ctx* ctx, const mdbn_rng* rng)
{
    REQUIRE(workspace_bytes >= need, "workspace %lld bytes < %lld needed (%s)", (long long)workspace_bytes, (long long)need, sizer);
    REQUIRE(ctx != nullptr && rng != nullptr, "ctx / rng is NULL");
    return MDBN_OK;
}

int sampler_pointer_rules(const void* workspace, std::initializer_list<const void*> optional_outputs)
{
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    for (const void* q : optional_outputs) REQUIRE(q == nullptr || aligned16(q), "output not 16-byte aligned");
    return MDBN_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------- annealed importance sampling
namespace {

// The clamp of mdbn_ais_cond_run: chain m of the N C chains keeps the columns where its data row's mask is 1 at obs.  A run
// without one (mdbn_ais_run) is the same run with no held column: one data row per chain, nothing to read.
struct AisClamp {
    const float* obs; const float* mask;
    int64_t mask_rows, N, C;
};

// The caller's workspace of an AIS run.  One-launch path: the visible state carried between launches.  General path: a
// zero bias (the propdown product is taken without bias), the pre-activations of a pass, the hidden and the visible state,
// s1 and d2 (mdbn_ais.hip: 64 floats, and under a clamp one sum per data row behind them), then the scratch of the
// propagation GEMMs.
struct AisWs {
    int64_t zero, pre, h, v, s1, d2, gemm_bytes;
    int64_t total_bytes() const { return 4 * (zero + pre + h + v + s1 + d2) + gemm_bytes; }
};

AisWs ais_ws(int path, int64_t M, int64_t clamp_rows, int64_t V, int64_t H, int64_t ldv, int64_t ldh)
{
    AisWs w{};
    w.v = ru64(M * ldv);
    w.d2 = 64;
    if (path == 2) {
        w.zero = ru64(std::max(ldv, ldh));
        w.pre = ru64(M * std::max(ldv, ldh));
        w.h = ru64(M * ldh);
        w.s1 = ru64(M);
        if (clamp_rows) w.d2 += ru64(clamp_rows);
        w.gemm_bytes = gemm_scratch_bytes(M, V, H, true);
    }
    return w;
}

// N C chains as mdbn_ais_run counts them
int cais_chain_rules(int64_t N, int64_t C, int64_t V, int64_t H)
{
    REQUIRE(N >= 1 && C >= 1 && V >= 1 && H >= 1, "bad shape N=%lld C=%lld V=%lld H=%lld", (long long)N, (long long)C, (long long)V, (long long)H);
    REQUIRE(N < (1ll << 31) && C < (1ll << 31) && N * C < (1ll << 31), "N C = %lld x %lld chains: too many", (long long)N, (long long)C);
    return MDBN_OK;
}

// What both sizers answer once their own shape rule holds: M chains, clamp_rows = the data rows of a clamp or 0
int ais_workspace_bytes(int64_t M, int64_t clamp_rows, int64_t V, int64_t H, int64_t n_betas, int path, int64_t* bytes)
{
    REQUIRE(n_betas >= 2, "n_betas = %lld: a schedule has at least beta_0 = 0 and beta_K = 1", (long long)n_betas);
    REQUIRE(path >= 0 && path <= 2, "path %d is not 0 (by shape), 1 (one launch) or 2 (general)", path);
    const int64_t ldv = padded_ld(V), ldh = padded_ld(H);
    const bool f0 = ais_small_ok(M, V, H, 0, ldv, ldh), f1 = ais_small_ok(M, V, H, 1, ldv, ldh);
    const int p = sizing_path(path, f0 || f1, f0 && f1);
    REQUIRE(p > 0, "path 1: %lld -> %lld is not LDS-resident", (long long)V, (long long)H);
    *bytes = ais_ws(p, M, clamp_rows, V, H, ldv, ldh).total_bytes();
    return MDBN_OK;
}

// The four runs once their own rules hold (the rules that need no device still come first): M chains, free (clamp == NULL)
// or clamped, each also on a layer with softmax groups (groups.on: the checked table of mdbn_ais_run_grouped /
// mdbn_ais_cond_run_grouped); `sizer` names the entry point's own *_workspace_bytes
int ais_run(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias, const float* vbias,
            const float* base_vbias, int gauss, const float* betas, int64_t n_betas, int64_t M, const AisClamp* clamp, int64_t ldv,
            float* v_state, double* logw, float* trace_h, float* trace_v, int path, const mdbn_rng* rng, void* workspace,
            int64_t workspace_bytes, const char* sizer, const AisGroups& groups = AisGroups{})
{
    REQUIRE(n_betas >= 2, "n_betas = %lld: a schedule has at least beta_0 = 0 and beta_K = 1", (long long)n_betas);
    if (clamp)
        REQUIRE(clamp->mask_rows == 1 || clamp->mask_rows == clamp->N, "mask_rows = %lld is neither 1 nor N = %lld",
                (long long)clamp->mask_rows, (long long)clamp->N);
    REQUIRE(path >= 0 && path <= 2, "path %d is not 0 (by shape), 1 (one launch) or 2 (general)", path);
    REQUIRE(ldv % 4 == 0 && ldv >= V && ldh % 4 == 0 && ldh >= H, "leading dimensions must be multiples of 4, ldv >= V, ldh >= H");
    const bool fits = ais_small_ok(M, V, H, gauss, ldv, ldh);
    REQUIRE(path != 1 || fits, "path 1: %lld -> %lld (ldv %lld, ldh %lld) is not LDS-resident", (long long)V, (long long)H,
            (long long)ldv, (long long)ldh);
    const int p = run_path(path, fits);
    const AisWs w = ais_ws(p, M, clamp ? clamp->N : 0, V, H, ldv, ldh);
    CHECK(sampler_workspace_rules(workspace_bytes, w.total_bytes(), sizer, ctx, rng));
    CHECK(check_mat(W, ldh, H, "W"));
    if (clamp) {
        CHECK(check_mat(clamp->obs, ldv, V, "obs"));
        CHECK(check_mat(clamp->mask, ldv, V, "mask"));
    }
    REQUIRE(hbias && vbias && base_vbias && betas && logw, "NULL pointer");
    CHECK(sampler_pointer_rules(workspace, {v_state, trace_h, trace_v}));
    hipStream_t s = (hipStream_t)stream;
    const int K = (int)n_betas - 1;
    float* wsf = reinterpret_cast<float*>(workspace);
    const float* obs = clamp ? clamp->obs : nullptr;
    const float* mask = clamp ? clamp->mask : nullptr;
    const int mask_rows = clamp ? (int)clamp->mask_rows : 1, C = clamp ? (int)clamp->C : 1;

    if (p == 1) {
        AisSmallArgs a{};
        a.M = (int)M; a.V = (int)V; a.H = (int)H; a.gauss = gauss != 0;
        a.ldv = ldv; a.ldh = ldh;
        a.W = W; a.hbias = hbias; a.vbias = vbias; a.base_vbias = base_vbias; a.betas = betas;
        a.K = K;
        a.rng = make_key(*rng, 0u);
        a.obs = obs; a.mask = mask; a.mask_rows = mask_rows; a.C = C;
        a.groups = groups;
        a.v_state = v_state ? v_state : wsf;
        a.logw = logw;
        a.trace_h = trace_h; a.trace_v = trace_v;
        for (int k0 = 0; k0 < K; k0 += AIS_CUT) {       // a launch stays short; the state travels in v_state / logw
            a.k0 = k0; a.k1 = std::min(K, k0 + AIS_CUT);
            HIP_OK(launch_ais_small(a, s));
        }
        return MDBN_OK;
    }

    float* zero = wsf;
    float* pre = zero + w.zero;
    float* h = pre + w.pre;
    float* v = h + w.h;
    float* s1 = v + w.v;
    float* d2 = s1 + w.s1;
    void* gemm_ws = d2 + w.d2;
    if (v_state) v = v_state;
    Workspace ws;
    CHECK(carve(gemm_ws, w.gemm_bytes, M, V, H, ws, false));
    HIP_OK(hipMemsetAsync(zero, 0, sizeof(float) * w.zero, s));
    AisStepArgs st{};
    st.M = (int)M; st.V = (int)V; st.H = (int)H; st.gauss = gauss != 0; st.K = K;
    st.ldv = ldv; st.ldh = ldh;
    st.betas = betas; st.vbias = vbias; st.base_vbias = base_vbias;
    st.rng = make_key(*rng, 0u);
    st.obs = obs; st.mask = mask; st.mask_rows = mask_rows; st.C = C;
    st.groups = groups;
    st.pre = pre; st.h = h; st.v = v; st.s1 = s1; st.d2 = d2; st.logw = logw;
    if (gauss) HIP_OK(launch_ais_d2(st, d2, s));         // (read under gauss only)
    st.k = 0; st.trace = trace_v;
    HIP_OK(launch_ais_visible(st, s));
    for (int k = 1; k <= K; ++k) {
        st.k = k;
        Affine up(v, M, ldv, W, V, H, ldh, hbias);
        up.pre = pre;
        // A held column may hold any real value: never the 0/1 operand hint on the way up under a clamp (where the state is 0/1
        // the six-product kernel adds exact zeros to the three products of the hinted one: the same bits)
        up.x_binary = !gauss && !clamp;
        CHECK(run_affine(up, ws, s, nullptr));
        st.trace = trace_h && k < K ? trace_h + (int64_t)(k - 1) * M * ldh : nullptr;
        HIP_OK(launch_ais_hidden(st, s));
        if (k == K) break;
        Affine down(h, M, ldh, W, V, H, ldh, zero, ldv, 1);
        down.pre = pre;
        down.x_binary = true;                            // our own 0/1 hidden samples
        CHECK(run_affine(down, ws, s, nullptr));
        st.trace = trace_v ? trace_v + (int64_t)k * M * ldv : nullptr;
        HIP_OK(launch_ais_visible(st, s));
    }
    return MDBN_OK;
}

}  // namespace

int mdbn_ais_workspace_bytes(mdbn_ctx* ctx, int64_t M, int64_t V, int64_t H, int64_t n_betas, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    REQUIRE(M >= 1 && V >= 1 && H >= 1, "bad shape M=%lld V=%lld H=%lld", (long long)M, (long long)V, (long long)H);
    return ais_workspace_bytes(M, 0, V, H, n_betas, path, bytes);
}

int mdbn_ais_run(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                 const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t n_betas, int64_t M,
                 int64_t ldv, float* v_state, double* logw, float* trace_h, float* trace_v, int path, const mdbn_rng* rng,
                 void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(M >= 1 && V >= 1 && H >= 1, "bad shape M=%lld V=%lld H=%lld", (long long)M, (long long)V, (long long)H);
    REQUIRE(M < (1ll << 31) && n_betas < (1ll << 30), "M / n_betas too large");
    return ais_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, gauss, betas, n_betas, M, nullptr, ldv, v_state, logw, trace_h,
                   trace_v, path, rng, workspace, workspace_bytes, "mdbn_ais_workspace_bytes");
}

int mdbn_ais_run_grouped(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                         const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t n_betas, int64_t M,
                         int64_t ldv, float* v_state, double* logw, float* trace_h, float* trace_v, int path, const mdbn_rng* rng,
                         void* workspace, int64_t workspace_bytes, const int32_t* group_start, const int32_t* group_start_host,
                         int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(M >= 1 && V >= 1 && H >= 1, "bad shape M=%lld V=%lld H=%lld", (long long)M, (long long)V, (long long)H);
    REQUIRE(M < (1ll << 31) && n_betas < (1ll << 30) && V <= (1 << 24), "M / n_betas / V too large");
    REQUIRE(!gauss, "categorical visible units: a Gaussian layer (gauss = 1) has no groups");
    AisGroups g{};
    CHECK(check_groups(group_start, group_start_host, n_groups, V, g.span_lo, g.span_hi));
    g.group_start = group_start; g.n_groups = (int)n_groups; g.on = 1;
    return ais_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, 0, betas, n_betas, M, nullptr, ldv, v_state, logw, trace_h,
                   trace_v, path, rng, workspace, workspace_bytes, "mdbn_ais_workspace_bytes", g);
}

int mdbn_ais_cond_workspace_bytes(mdbn_ctx* ctx, int64_t N, int64_t C, int64_t V, int64_t H, int64_t n_betas, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    CHECK(cais_chain_rules(N, C, V, H));
    return ais_workspace_bytes(N * C, N, V, H, n_betas, path, bytes);
}

int mdbn_ais_cond_run(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                      const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t n_betas,
                      const float* obs, const float* mask, int64_t mask_rows, int64_t N, int64_t C, int64_t ldv, float* v_state,
                      double* logw, float* trace_h, float* trace_v, int path, const mdbn_rng* rng, void* workspace,
                      int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    CHECK(cais_chain_rules(N, C, V, H));
    REQUIRE(n_betas < (1ll << 30), "n_betas too large");
    const AisClamp clamp{obs, mask, mask_rows, N, C};
    return ais_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, gauss, betas, n_betas, N * C, &clamp, ldv, v_state, logw,
                   trace_h, trace_v, path, rng, workspace, workspace_bytes, "mdbn_ais_cond_workspace_bytes");
}

int mdbn_ais_cond_run_grouped(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                              const float* vbias, const float* base_vbias, const float* betas, int64_t n_betas, const float* obs,
                              const float* mask, int64_t mask_rows, int64_t N, int64_t C, int64_t ldv, float* v_state,
                              double* logw, float* trace_h, float* trace_v, int path, const mdbn_rng* rng, void* workspace,
                              int64_t workspace_bytes, const int32_t* group_start, const int32_t* group_start_host,
                              int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    CHECK(cais_chain_rules(N, C, V, H));
    REQUIRE(n_betas < (1ll << 30) && V <= (1 << 24), "n_betas / V too large");
    AisGroups g{};
    CHECK(check_groups(group_start, group_start_host, n_groups, V, g.span_lo, g.span_hi));
    g.group_start = group_start; g.n_groups = (int)n_groups; g.on = 1;
    const AisClamp clamp{obs, mask, mask_rows, N, C};
    return ais_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, 0, betas, n_betas, N * C, &clamp, ldv, v_state, logw,
                   trace_h, trace_v, path, rng, workspace, workspace_bytes, "mdbn_ais_cond_workspace_bytes", g);
}

// ---------------------------------------------------------------------------------- clamped Gibbs sampling
namespace {

// The caller's workspace of mdbn_gibbs_clamped: the two accumulators (one-launch path: what a cut run carries from launch to
// launch), then -- general path -- the scratch of the propagation GEMMs.
struct ClampWs {
    int64_t acc_v, acc_h, gemm_bytes;
    int64_t total_bytes() const { return 4 * (acc_v + acc_h) + gemm_bytes; }
};

ClampWs clamp_ws(int path, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh)
{
    ClampWs w{};
    w.acc_v = ru64(B * ldv);
    w.acc_h = ru64(B * ldh);
    if (path == 2) w.gemm_bytes = gemm_scratch_bytes(B, V, H, false);
    return w;
}

}  // namespace

int mdbn_gibbs_clamped_workspace_bytes(mdbn_ctx* ctx, int64_t B, int64_t V, int64_t H, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    REQUIRE(B >= 1 && V >= 1 && H >= 1, "bad shape B=%lld V=%lld H=%lld", (long long)B, (long long)V, (long long)H);
    REQUIRE(path >= 0 && path <= 2, "path %d is not 0 (by shape), 1 (one launch) or 2 (general)", path);
    const int64_t ldv = padded_ld(V), ldh = padded_ld(H);
    const bool f0 = clamp_small_ok(B, V, H, 0, ldv, ldh), f1 = clamp_small_ok(B, V, H, 1, ldv, ldh);
    const int p = sizing_path(path, f0 || f1, f0 && f1);
    REQUIRE(p > 0, "path 1: %lld -> %lld is not LDS-resident", (long long)V, (long long)H);
    *bytes = clamp_ws(p, B, V, H, ldv, ldh).total_bytes();
    return MDBN_OK;
}

namespace {

// Both runs once their own rules hold: the plain chain, or (groups.on: the checked table of mdbn_gibbs_clamped_grouped) the
// chain of a Bernoulli layer with softmax groups
int clamp_run(mdbn_ctx* ctx, void* stream, float* v, const float* obs, const float* mask, int64_t mask_rows,
              int64_t B, int64_t ldv, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
              const float* vbias, int gauss, int add_noise, int64_t n_steps, int64_t burn_in, float* h_mean,
              float* h_sample, float* v_mean, float* v_avg, float* h_avg, float* trace_h, float* trace_v,
              int path, int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes,
              const ClampGroups& groups = ClampGroups{})
{
    REQUIRE(n_steps >= 1 && n_steps < (1ll << 30), "n_steps = %lld must be in [1, 2^30)", (long long)n_steps);
    REQUIRE(burn_in >= 0 && burn_in < n_steps, "burn_in = %lld must be in [0, n_steps = %lld)", (long long)burn_in, (long long)n_steps);
    REQUIRE(mask_rows == 1 || mask_rows == B, "mask_rows = %lld is neither 1 nor B = %lld", (long long)mask_rows, (long long)B);
    REQUIRE(gauss >= 0 && gauss <= 2, "gauss = %d is not 0 (Bernoulli), 1 (Gaussian, hidden mean down) or 2 (Gaussian, Gibbs sampler)", gauss);
    REQUIRE(path >= 0 && path <= 2, "path %d is not 0 (by shape), 1 (one launch) or 2 (general)", path);
    REQUIRE(steps_per_launch >= 0, "steps_per_launch = %lld is negative (0 = default)", (long long)steps_per_launch);
    REQUIRE(ldv % 4 == 0 && ldv >= V && ldh % 4 == 0 && ldh >= H, "leading dimensions must be multiples of 4, ldv >= V, ldh >= H");
    const bool fits = clamp_small_ok(B, V, H, gauss, ldv, ldh);
    REQUIRE(path != 1 || fits, "path 1: %lld -> %lld (ldv %lld, ldh %lld) is not LDS-resident", (long long)V, (long long)H,
            (long long)ldv, (long long)ldh);
    const int p = run_path(path, fits);
    const ClampWs w = clamp_ws(p, B, V, H, ldv, ldh);
    CHECK(sampler_workspace_rules(workspace_bytes, w.total_bytes(), "mdbn_gibbs_clamped_workspace_bytes", ctx, rng));
    CHECK(check_mat(v, ldv, V, "v"));
    CHECK(check_mat(obs, ldv, V, "obs"));
    CHECK(check_mat(mask, ldv, V, "mask"));
    CHECK(check_mat(W, ldh, H, "W"));
    CHECK(check_mat(h_mean, ldh, H, "h_mean"));
    CHECK(check_mat(h_sample, ldh, H, "h_sample"));
    CHECK(check_mat(v_mean, ldv, V, "v_mean"));
    REQUIRE(hbias && vbias, "bias pointers are NULL");
    CHECK(sampler_pointer_rules(workspace, {v_avg, h_avg, trace_h, trace_v}));
    hipStream_t s = (hipStream_t)stream;
    float* acc_v = reinterpret_cast<float*>(workspace);
    float* acc_h = acc_v + w.acc_v;
    const bool noisy = gauss && (add_noise || gauss == 2);
    const bool feed_sample = gauss != 1;            // gauss = 1: the hidden MEAN goes down (mdbn_gibbs_chain); 2: the sample

    if (p == 1) {
        ClampSmallArgs a{};
        a.B = (int)B; a.V = (int)V; a.H = (int)H; a.gauss = gauss; a.add_noise = add_noise != 0;
        a.ldv = ldv; a.ldh = ldh;
        a.W = W; a.hbias = hbias; a.vbias = vbias;
        a.v = v; a.obs = obs; a.mask = mask; a.mask_rows = (int)mask_rows;
        a.n_steps = (int)n_steps; a.burn_in = (int)burn_in;
        a.rng = make_key(*rng, 0u);
        a.h_mean = h_mean; a.h_sample = h_sample; a.v_mean = v_mean; a.v_avg = v_avg; a.h_avg = h_avg;
        a.acc_v = acc_v; a.acc_h = acc_h;
        a.trace_h = trace_h; a.trace_v = trace_v;
        a.groups = groups;
        const int64_t cut = steps_per_launch ? steps_per_launch : CLAMP_CUT;
        for (int64_t t0 = 0; t0 < n_steps; t0 += cut) {       // a launch stays short; the state travels in v / acc_v / acc_h
            a.t0 = (int)t0; a.t1 = (int)std::min(n_steps, t0 + cut);
            HIP_OK(launch_clamp_small(a, s));
        }
        return MDBN_OK;
    }

    Workspace ws;
    CHECK(carve(acc_h + w.acc_h, w.gemm_bytes, B, V, H, ws, false));
    HIP_OK(hipMemsetAsync(acc_v, 0, sizeof(float) * (w.acc_v + w.acc_h), s));
    ClampStepArgs c{};
    c.B = (int)B; c.V = (int)V; c.H = (int)H;
    c.ldv = ldv; c.ldh = ldh;
    c.v = v; c.v_mean = v_mean; c.obs = obs; c.mask = mask; c.mask_rows = (int)mask_rows;
    c.h_mean = h_mean; c.h_sample = h_sample;
    c.n_avg = (float)(n_steps - burn_in);
    c.acc_v = acc_v; c.acc_h = acc_h; c.v_avg = v_avg; c.h_avg = h_avg;
    c.entry = 1; c.v_new = v;
    ClampStepGroupedArgs cg{};
    cg.groups = groups;
    if (groups.on) {
        cg.c = c;
        HIP_OK(launch_clamp_step_grouped(cg, s));
    } else {
        HIP_OK(launch_clamp_step(c, s));
    }
    c.entry = 0;
    for (int64_t t = 0; t < n_steps; ++t) {
        const bool last = t + 1 == n_steps;
        mdbn_rng rh = *rng, rv = *rng;
        rh.step = rng->step + (uint32_t)(2 * t);     rh.draw = 0;
        rv.step = rng->step + (uint32_t)(2 * t + 1); rv.draw = 0;
        if (groups.on) {
            // the propup of the plain chain; the propdown to the LINEAR pre-activations h_sample W^T + vbias, into v_mean (as
            // mdbn_cd_step_grouped forms them); then the draw, the clamp, the accumulators and the taps in one kernel
            Affine up(v, B, ldv, W, V, H, ldh, hbias);
            up.mean = h_mean; up.sample = h_sample; up.rng = &rh;
            CHECK(run_affine(up, ws, s, nullptr));
            Affine down(h_sample, B, ldh, W, V, H, ldh, vbias, ldv, 1);
            down.mean = v_mean;
            down.x_binary = true;                        // our own 0/1 hidden samples
            CHECK(run_affine(down, ws, s, nullptr));
            c.accumulate = t >= burn_in; c.last = last;
            c.trace_h = trace_h ? trace_h + t * B * ldh : nullptr;
            c.trace_v = trace_v ? trace_v + t * B * ldv : nullptr;
            cg.c = c;
            cg.rng = make_key(rv, 0u);
            HIP_OK(launch_clamp_step_grouped(cg, s));
            continue;
        }
        // the passes of mdbn_gibbs_chain.  The visible state may hold real observed values: never the 0/1 operand hint there
        Affine up(v, B, ldv, W, V, H, ldh, hbias);
        up.mean = h_mean; up.sample = (feed_sample || last || trace_h) ? h_sample : nullptr; up.rng = &rh;
        CHECK(run_affine(up, ws, s, nullptr));
        Affine down(feed_sample ? h_sample : h_mean, B, ldh, W, V, H, ldh, vbias, ldv, gauss != 0);
        down.mean = v_mean; down.sample = (!gauss || noisy) ? v : nullptr; down.rng = &rv;
        down.x_binary = feed_sample;                     // our own 0/1 hidden samples
        CHECK(run_affine(down, ws, s, nullptr));
        c.v_new = (!gauss || noisy) ? v : v_mean;
        c.accumulate = t >= burn_in; c.last = last;
        c.trace_h = trace_h ? trace_h + t * B * ldh : nullptr;
        c.trace_v = trace_v ? trace_v + t * B * ldv : nullptr;
        HIP_OK(launch_clamp_step(c, s));
    }
    return MDBN_OK;
}

}  // namespace

int mdbn_gibbs_clamped(mdbn_ctx* ctx, void* stream, float* v, const float* obs, const float* mask, int64_t mask_rows,
                       int64_t B, int64_t ldv, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                       const float* vbias, int gauss, int add_noise, int64_t n_steps, int64_t burn_in, float* h_mean,
                       float* h_sample, float* v_mean, float* v_avg, float* h_avg, float* trace_h, float* trace_v,
                       int path, int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    // (the argument rules first: they need no device)
    REQUIRE(B >= 1 && V >= 1 && H >= 1, "bad shape B=%lld V=%lld H=%lld", (long long)B, (long long)V, (long long)H);
    REQUIRE(B < (1ll << 31), "B too large");
    return clamp_run(ctx, stream, v, obs, mask, mask_rows, B, ldv, W, V, H, ldh, hbias, vbias, gauss, add_noise, n_steps, burn_in,
                     h_mean, h_sample, v_mean, v_avg, h_avg, trace_h, trace_v, path, steps_per_launch, rng, workspace, workspace_bytes);
}

int mdbn_gibbs_clamped_grouped(mdbn_ctx* ctx, void* stream, float* v, const float* obs, const float* mask, int64_t mask_rows,
                               int64_t B, int64_t ldv, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                               const float* vbias, int64_t n_steps, int64_t burn_in, float* h_mean, float* h_sample,
                               float* v_mean, float* v_avg, float* h_avg, float* trace_h, float* trace_v, int path,
                               int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes,
                               const int32_t* group_start, const int32_t* group_start_host, int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(B >= 1 && V >= 1 && H >= 1, "bad shape B=%lld V=%lld H=%lld", (long long)B, (long long)V, (long long)H);
    REQUIRE(B < (1ll << 31) && V <= (1 << 24), "B / V too large");
    ClampGroups g{};
    CHECK(check_groups(group_start, group_start_host, n_groups, V, g.span_lo, g.span_hi));
    g.group_start = group_start; g.n_groups = (int)n_groups; g.on = 1;
    return clamp_run(ctx, stream, v, obs, mask, mask_rows, B, ldv, W, V, H, ldh, hbias, vbias, 0, 0, n_steps, burn_in, h_mean,
                     h_sample, v_mean, v_avg, h_avg, trace_h, trace_v, path, steps_per_launch, rng, workspace, workspace_bytes, g);
}

// ---------------------------------------------------------------------------------- parallel tempering
namespace {

// The caller's workspace of mdbn_pt_run: the betas on the device, the per-ladder swap counts and the two running sums (what a
// cut run carries from launch to launch), then -- general path -- a zero bias, the pre-activations of a pass, s1
// (mdbn_temper.hip) and the scratch of the propagation GEMMs over M R rows.  mdbn_pt_run_z (`z`): on the general path also
// g = |b - b_A|^2, a double, behind the running sums.
struct PtWs {
    int64_t betas, counts, v_sum, h_sum, g, zero, pre, s1, gemm_bytes;
    int64_t total_bytes() const { return 4 * (betas + counts + v_sum + h_sum + g + zero + pre + s1) + gemm_bytes; }
};

PtWs pt_ws(int path, int64_t M, int64_t R, int64_t V, int64_t H, int64_t ldv, int64_t ldh, bool z = false)
{
    PtWs w{};
    w.betas = ru64(R);
    w.counts = ru64(M * (R - 1));
    w.v_sum = ru64(M * ldv);
    w.h_sum = ru64(M * ldh);
    if (path == 2 && z) w.g = ru64(2);
    if (path == 2) {
        const int64_t rows = M * R;
        w.zero = ru64(std::max(ldv, ldh));
        w.pre = ru64(rows * std::max(ldv, ldh));
        w.s1 = ru64(rows);
        w.gemm_bytes = gemm_scratch_bytes(rows, V, H, true);
    }
    return w;
}

}  // namespace

namespace {

int pt_workspace_bytes(mdbn_ctx* ctx, int64_t M, int64_t R, int64_t V, int64_t H, int path, int64_t* bytes, bool z)
{
    REQUIRE(bytes != nullptr, "bytes is NULL");
    REQUIRE(M >= 1 && V >= 1 && H >= 1, "bad shape M=%lld V=%lld H=%lld", (long long)M, (long long)V, (long long)H);
    REQUIRE(R >= 2 && R <= PT_MAX_R_GENERAL, "R = %lld: a ladder has 2 to %d temperatures", (long long)R, PT_MAX_R_GENERAL);
    REQUIRE(M * R < (1ll << 31), "M * R too large");
    REQUIRE(path >= 0 && path <= 2, "path %d is not 0 (by shape), 1 (one launch) or 2 (general)", path);
    const int64_t ldv = padded_ld(V), ldh = padded_ld(H);
    const int p = sizing_path(path, pt_small_ok(M, R, V, H, 0, ldv, ldh) || pt_small_ok(M, R, V, H, 1, ldv, ldh),
                              pt_small_preferred(M, R, V, H, 0, ldv, ldh) && pt_small_preferred(M, R, V, H, 1, ldv, ldh));
    REQUIRE(p > 0, "path 1: %lld -> %lld with R = %lld is not LDS-resident (or R is no multiple of 4)", (long long)V, (long long)H,
            (long long)R);
    *bytes = pt_ws(p, M, R, V, H, ldv, ldh, z).total_bytes();
    return MDBN_OK;
}

// mdbn_pt_run (z = false: zacc and trace_work NULL), mdbn_pt_run_z and (groups.on: the checked table of mdbn_pt_run_grouped,
// gauss = 0) the run of a Bernoulli layer with softmax groups: one statement of the rules and of the run
int pt_run(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
           const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t R, int64_t M, int64_t ldv,
           float* v, float* h, int32_t* rank, int64_t n_sweeps, int64_t burn_in, int64_t sweep0, int32_t* accepted,
           float* v_avg, float* h_avg, float* trace_v, float* trace_h, int32_t* trace_swaps, int path,
           int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes, bool z, double* zacc,
           double* trace_work, const AisGroups& groups = AisGroups{})
{
    // (the argument rules first: they need no device)
    REQUIRE(M >= 1 && V >= 1 && H >= 1, "bad shape M=%lld V=%lld H=%lld", (long long)M, (long long)V, (long long)H);
    REQUIRE(R >= 2 && R <= PT_MAX_R_GENERAL, "R = %lld: a ladder has 2 to %d temperatures", (long long)R, PT_MAX_R_GENERAL);
    REQUIRE(M * R < (1ll << 31), "M * R too large");
    REQUIRE(betas != nullptr, "betas is NULL (a host array of R values)");
    REQUIRE(betas[0] >= 0.0f, "betas[0] = %g is negative", (double)betas[0]);
    for (int64_t r = 1; r < R; ++r)
        REQUIRE(betas[r] > betas[r - 1], "betas must rise strictly: betas[%lld] = %g after %g", (long long)r, (double)betas[r],
                (double)betas[r - 1]);
    REQUIRE(betas[R - 1] == 1.0f, "betas must end at exactly 1, not %.9g", (double)betas[R - 1]);
    REQUIRE(n_sweeps >= 1 && n_sweeps < (1ll << 29), "n_sweeps = %lld must be in [1, 2^29)", (long long)n_sweeps);
    REQUIRE(burn_in >= 0 && burn_in < n_sweeps, "burn_in = %lld must be in [0, n_sweeps = %lld)", (long long)burn_in, (long long)n_sweeps);
    REQUIRE(sweep0 >= 0, "sweep0 = %lld is negative", (long long)sweep0);
    REQUIRE(gauss == 0 || gauss == 1, "gauss = %d is not 0 (Bernoulli) or 1 (Gaussian visibles)", gauss);
    REQUIRE(path >= 0 && path <= 2, "path %d is not 0 (by shape), 1 (one launch) or 2 (general)", path);
    REQUIRE(steps_per_launch >= 0, "steps_per_launch = %lld is negative (0 = default)", (long long)steps_per_launch);
    REQUIRE(ldv % 4 == 0 && ldv >= V && ldh % 4 == 0 && ldh >= H, "leading dimensions must be multiples of 4, ldv >= V, ldh >= H");
    const bool fits = pt_small_ok(M, R, V, H, gauss, ldv, ldh);
    REQUIRE(path != 1 || fits, "path 1: %lld -> %lld (ldv %lld, ldh %lld) with R = %lld is not LDS-resident (or R is no multiple of 4)",
            (long long)V, (long long)H, (long long)ldv, (long long)ldh, (long long)R);
    // (path = 0: the one-launch kernel only where it was measured to win: pt_small_preferred)
    const int p = run_path(path, pt_small_preferred(M, R, V, H, gauss, ldv, ldh));
    const PtWs w = pt_ws(p, M, R, V, H, ldv, ldh, z);
    CHECK(sampler_workspace_rules(workspace_bytes, w.total_bytes(), z ? "mdbn_pt_run_z_workspace_bytes" : "mdbn_pt_workspace_bytes", ctx, rng));
    CHECK(check_mat(W, ldh, H, "W"));
    CHECK(check_mat(v, ldv, V, "v"));
    CHECK(check_mat(h, ldh, H, "h"));
    REQUIRE(hbias && vbias && base_vbias && rank && accepted, "NULL pointer");
    CHECK(sampler_pointer_rules(workspace, {v_avg, h_avg, trace_h, trace_v, zacc, trace_work}));
    hipStream_t s = (hipStream_t)stream;
    float* wsf = reinterpret_cast<float*>(workspace);
    float* d_betas = wsf;
    int* counts = reinterpret_cast<int*>(d_betas + w.betas);
    float* v_sum = reinterpret_cast<float*>(counts) + w.counts;
    float* h_sum = v_sum + w.v_sum;
    HIP_OK(hipMemcpyAsync(d_betas, betas, sizeof(float) * R, hipMemcpyHostToDevice, s));

    if (p == 1) {
        PtSmallArgs a{};
        a.M = (int)M; a.R = (int)R; a.V = (int)V; a.H = (int)H; a.gauss = gauss;
        a.ldv = ldv; a.ldh = ldh;
        a.W = W; a.hbias = hbias; a.vbias = vbias; a.base_vbias = base_vbias; a.betas = d_betas;
        a.v = v; a.h = h; a.rank = rank; a.counts = counts;
        a.v_sum = v_sum; a.h_sum = h_sum; a.v_avg = v_avg; a.h_avg = h_avg;
        a.n = (int)n_sweeps; a.burn_in = (int)burn_in; a.sweep0 = sweep0;
        a.rng = make_key(*rng, 0u);
        a.trace_v = trace_v; a.trace_h = trace_h; a.trace_swaps = trace_swaps;
        a.zacc = zacc; a.trace_work = trace_work;
        a.groups = groups;
        const int64_t cut = steps_per_launch ? steps_per_launch : pt_default_cut(R);
        for (int64_t t0 = 0; t0 < n_sweeps; t0 += cut) {      // a launch stays short; the state travels in h / rank / counts / sums
            a.t0 = (int)t0; a.t1 = (int)std::min(n_sweeps, t0 + cut);
            HIP_OK(launch_pt_small(a, s));
        }
        HIP_OK(launch_pt_counts(counts, (int)M, (int)R, accepted, s));
        return MDBN_OK;
    }

    const int64_t rows = M * R;
    double* g = reinterpret_cast<double*>(h_sum + w.h_sum);
    float* zero = h_sum + w.h_sum + w.g;
    float* pre = zero + w.zero;
    float* s1 = pre + w.pre;
    void* gemm_ws = s1 + w.s1;
    Workspace ws;
    CHECK(carve(gemm_ws, w.gemm_bytes, rows, V, H, ws, false));
    HIP_OK(hipMemsetAsync(counts, 0, sizeof(float) * (w.counts + w.v_sum + w.h_sum + w.g + w.zero), s));
    PtStepArgs st{};
    st.M = (int)M; st.R = (int)R; st.V = (int)V; st.H = (int)H; st.gauss = gauss;
    st.ldv = ldv; st.ldh = ldh;
    st.vbias = vbias; st.base_vbias = base_vbias; st.betas = d_betas;
    st.pre = pre; st.v = v; st.h = h; st.rank = rank; st.counts = counts; st.s1 = s1;
    st.v_sum = v_sum; st.h_sum = h_sum; st.v_avg = v_avg; st.h_avg = h_avg;
    st.n_avg = (float)(n_sweeps - burn_in); st.sweep0 = sweep0;
    st.rng = make_key(*rng, 0u);
    st.zacc = zacc;
    st.groups = groups;
    if (zacc || trace_work) {
        st.g = g;
        if (gauss) HIP_OK(launch_pt_gnorm(vbias, base_vbias, (int)V, g, s));
    }
    for (int64_t t = 0; t < n_sweeps; ++t) {
        st.t = (int)t; st.accumulate = t >= burn_in; st.last = t + 1 == n_sweeps;
        st.trace_work = trace_work ? trace_work + t * M * (R - 1) * 2 : nullptr;
        st.trace_v = trace_v ? trace_v + t * rows * ldv : nullptr;
        st.trace_h = trace_h ? trace_h + t * rows * ldh : nullptr;
        st.trace_swaps = trace_swaps ? trace_swaps + t * M * 2 * R : nullptr;
        Affine down(h, rows, ldh, W, V, H, ldh, zero, ldv, 1);
        down.pre = pre;
        down.x_binary = true;                            // our own 0/1 hidden samples
        CHECK(run_affine(down, ws, s, nullptr));
        HIP_OK(launch_pt_visible(st, s));
        Affine up(v, rows, ldv, W, V, H, ldh, hbias);
        up.pre = pre;
        up.x_binary = !gauss;
        CHECK(run_affine(up, ws, s, nullptr));
        HIP_OK(launch_pt_swap_hidden(st, s));
    }
    HIP_OK(launch_pt_counts(counts, (int)M, (int)R, accepted, s));
    return MDBN_OK;
}

}  // namespace

int mdbn_pt_workspace_bytes(mdbn_ctx* ctx, int64_t M, int64_t R, int64_t V, int64_t H, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    return pt_workspace_bytes(ctx, M, R, V, H, path, bytes, false);
}

int mdbn_pt_run_z_workspace_bytes(mdbn_ctx* ctx, int64_t M, int64_t R, int64_t V, int64_t H, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    return pt_workspace_bytes(ctx, M, R, V, H, path, bytes, true);
}

int mdbn_pt_run(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t R, int64_t M, int64_t ldv,
                float* v, float* h, int32_t* rank, int64_t n_sweeps, int64_t burn_in, int64_t sweep0, int32_t* accepted,
                float* v_avg, float* h_avg, float* trace_v, float* trace_h, int32_t* trace_swaps, int path,
                int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    return pt_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, gauss, betas, R, M, ldv, v, h, rank, n_sweeps, burn_in, sweep0,
                  accepted, v_avg, h_avg, trace_v, trace_h, trace_swaps, path, steps_per_launch, rng, workspace, workspace_bytes, false,
                  nullptr, nullptr);
}

int mdbn_pt_run_z(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                  const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t R, int64_t M, int64_t ldv,
                  float* v, float* h, int32_t* rank, int64_t n_sweeps, int64_t burn_in, int64_t sweep0, int32_t* accepted,
                  float* v_avg, float* h_avg, float* trace_v, float* trace_h, int32_t* trace_swaps, int path,
                  int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes, double* zacc,
                  double* trace_work)
{
    CtxScope ctx_scope(ctx);
    return pt_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, gauss, betas, R, M, ldv, v, h, rank, n_sweeps, burn_in, sweep0,
                  accepted, v_avg, h_avg, trace_v, trace_h, trace_swaps, path, steps_per_launch, rng, workspace, workspace_bytes, true,
                  zacc, trace_work);
}

int mdbn_pt_run_grouped(mdbn_ctx* ctx, void* stream, const float* W, int64_t V, int64_t H, int64_t ldh, const float* hbias,
                        const float* vbias, const float* base_vbias, int gauss, const float* betas, int64_t R, int64_t M,
                        int64_t ldv, float* v, float* h, int32_t* rank, int64_t n_sweeps, int64_t burn_in, int64_t sweep0,
                        int32_t* accepted, float* v_avg, float* h_avg, float* trace_v, float* trace_h, int32_t* trace_swaps,
                        int path, int64_t steps_per_launch, const mdbn_rng* rng, void* workspace, int64_t workspace_bytes,
                        double* zacc, double* trace_work, const int32_t* group_start, const int32_t* group_start_host,
                        int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(M >= 1 && V >= 1 && H >= 1, "bad shape M=%lld V=%lld H=%lld", (long long)M, (long long)V, (long long)H);
    REQUIRE(V <= (1 << 24), "V too large");
    REQUIRE(!gauss, "categorical visible units: a Gaussian layer (gauss = 1) has no groups");
    AisGroups g{};
    CHECK(check_groups(group_start, group_start_host, n_groups, V, g.span_lo, g.span_hi));
    g.group_start = group_start; g.n_groups = (int)n_groups; g.on = 1;
    return pt_run(ctx, stream, W, V, H, ldh, hbias, vbias, base_vbias, 0, betas, R, M, ldv, v, h, rank, n_sweeps, burn_in, sweep0,
                  accepted, v_avg, h_avg, trace_v, trace_h, trace_swaps, path, steps_per_launch, rng, workspace, workspace_bytes, true,
                  zacc, trace_work, g);
}

// ---------------------------------------------------------------------------------- variational bound (mdbn_bound.hip)
int mdbn_rowll_workspace_bytes(mdbn_ctx* ctx, int64_t R, int64_t V, int64_t H, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && bytes && R > 0 && V > 0 && H > 0, "bad arguments");
    *bytes = rowll_partial_floats(R, V) * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_propdown_rowll(mdbn_ctx* ctx, void* stream, const float* h, int64_t R, int64_t ldh, const float* W, int64_t V, int64_t H,
                        const float* vbias, const float* target, int64_t ldv, int64_t target_div, int gauss, float* out,
                        void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && h && W && vbias && target && out && R > 0 && V > 0 && H > 0, "bad arguments");
    REQUIRE(R <= (1 << 30) && V <= (1 << 30) && H <= (1 << 30), "shape too large");
    REQUIRE(target_div >= 1 && target_div <= (1 << 30), "target_div must be >= 1");
    REQUIRE(ldh >= H && ldv >= V && ldh % 4 == 0, "leading dimensions: ldh >= H, ldh %% 4 == 0, ldv >= V");
    REQUIRE(aligned16(h) && aligned16(W), "h and W must be 16-byte aligned");
    RowllArgs a;
    a.R = (int)R; a.V = (int)V; a.H = (int)H; a.gauss = gauss != 0; a.target_div = (int)target_div;
    a.tiles_m = (int)((R + ROWLL_BM - 1) / ROWLL_BM); a.tiles_n = (int)((V + ROWLL_BN - 1) / ROWLL_BN);
    REQUIRE((int64_t)a.tiles_m * a.tiles_n <= 0x7fffffff, "shape too large");
    REQUIRE(workspace != nullptr && workspace_bytes >= rowll_partial_floats(R, V) * (int64_t)sizeof(float),
            "workspace of mdbn_rowll_workspace_bytes needed");
    a.ldh = ldh; a.ldv = ldv; a.h = h; a.W = W; a.vbias = vbias; a.target = target;
    a.partial = reinterpret_cast<float*>(workspace); a.out = out;
    HIP_OK(launch_rowll(a, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_rowll_grouped_workspace_bytes(mdbn_ctx* ctx, int64_t R, int64_t V, int64_t H, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && bytes && R > 0 && V > 0 && H > 0, "bad arguments");
    *bytes = rowll_grouped_partial_floats(R, V) * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_propdown_rowll_grouped(mdbn_ctx* ctx, void* stream, const float* h, int64_t R, int64_t ldh, const float* W, int64_t V,
                                int64_t H, const float* vbias, const float* target, int64_t ldv, int64_t target_div, float* out,
                                void* workspace, int64_t workspace_bytes, const int32_t* group_start,
                                const int32_t* group_start_host, int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && h && W && vbias && target && out && R > 0 && V > 0 && H > 0, "bad arguments");
    REQUIRE(R <= (1 << 30) && V <= (1 << 24) && H <= (1 << 30), "shape too large");
    REQUIRE(target_div >= 1 && target_div <= (1 << 30), "target_div must be >= 1");
    REQUIRE(ldh >= H && ldv >= V && ldh % 4 == 0, "leading dimensions: ldh >= H, ldh %% 4 == 0, ldv >= V");
    REQUIRE(aligned16(h) && aligned16(W), "h and W must be 16-byte aligned");
    REQUIRE(n_groups >= 1, "n_groups = %lld: a layer without groups goes through mdbn_propdown_rowll", (long long)n_groups);
    RowllGroupArgs g;
    CHECK(check_groups(group_start, group_start_host, n_groups, V, g.span_lo, g.span_hi));
    g.group_start = group_start; g.n_groups = (int)n_groups;
    RowllArgs& a = g.a;
    a.R = (int)R; a.V = (int)V; a.H = (int)H; a.gauss = 0; a.target_div = (int)target_div;
    a.tiles_m = (int)((R + ROWLL_BM - 1) / ROWLL_BM); a.tiles_n = (int)((V + ROWLL_BN - 1) / ROWLL_BN);
    REQUIRE((int64_t)a.tiles_m * a.tiles_n <= 0x7fffffff, "shape too large");
    REQUIRE(workspace != nullptr && workspace_bytes >= rowll_grouped_partial_floats(R, V) * (int64_t)sizeof(float),
            "workspace of mdbn_rowll_grouped_workspace_bytes needed");
    a.ldh = ldh; a.ldv = ldv; a.h = h; a.W = W; a.vbias = vbias; a.target = target;
    a.partial = reinterpret_cast<float*>(workspace); a.out = out;
    HIP_OK(launch_rowll_grouped(g, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_sample_replicas(mdbn_ctx* ctx, void* stream, const float* mean, int64_t N, int64_t H, int64_t ldh, int64_t S,
                         float* sample, float* entropy, const mdbn_rng* rng)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && mean && sample && rng && N > 0 && H > 0 && S > 0 && ldh >= H, "bad arguments");
    REQUIRE(N <= ((int64_t)1 << 40) / S && rng->row_offset <= ((uint64_t)1 << 40), "shape too large");
    ReplicaArgs a;
    a.N = N; a.S = S; a.H = H; a.ldh = ldh; a.mean = mean; a.sample = sample; a.entropy = entropy;
    a.rng = make_key(*rng, rng->draw);
    HIP_OK(launch_sample_replicas(a, (hipStream_t)stream));
    return MDBN_OK;
}

}  // extern "C"

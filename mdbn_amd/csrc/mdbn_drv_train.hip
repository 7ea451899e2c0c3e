// C-ABI drivers of the training add-ons (declared in include/mdbn_hip.h): centred CD (mdbn_center.hip), the sparsity target
// (mdbn_sparsity.hip) and up-down fine-tuning (mdbn_updown.hip).  Of the core they use what mdbn_capi_internal.h declares and
// the public entry points mdbn_cd_stats / mdbn_apply_update.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "mdbn_capi_internal.h"
#include "mdbn_thin.h"
#include "mdbn_center.h"
#include "mdbn_sparsity.h"
#include "mdbn_updown.h"

using namespace mdbn;
using namespace mdbn::capi;

extern "C" {

// ---------------------------------------------------------------------------------- centred CD (mdbn_center.hip)
int mdbn_center_workspace_bytes(mdbn_ctx* ctx, int64_t V, int64_t H, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && bytes && V > 0 && H > 0 && V <= (1 << 30) && H <= CENTER_MAX_H, "bad arguments (0 < V <= 2^30, 0 < H <= %d)", CENTER_MAX_H);
    *bytes = center_partial_floats(V, H) * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_center_offsets(mdbn_ctx* ctx, void* stream, const float* v0, int64_t ldv, const float* ph, int64_t ldh, int64_t B,
                        int64_t V, int64_t H, float nu, float* mu, float* lam)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && v0 && ph && mu && lam, "null pointer");
    REQUIRE(B > 0 && V > 0 && H > 0 && B <= (1 << 30) && V <= (1 << 30) && H <= (1 << 30), "sizes must be positive (and <= 2^30)");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
    REQUIRE(aligned16(v0) && aligned16(ph), "v0 and ph must be 16-byte aligned");
    REQUIRE((reinterpret_cast<uintptr_t>(mu) & 3u) == 0 && (reinterpret_cast<uintptr_t>(lam) & 3u) == 0, "mu / lam not aligned");
    REQUIRE(nu > 0.f && nu <= 1.f, "nu must lie in (0, 1]");
    CenterOffsetsArgs a;
    a.v0 = v0; a.ph = ph; a.ldv = ldv; a.ldh = ldh; a.B = (int)B; a.V = (int)V; a.H = (int)H; a.nu = nu; a.mu = mu; a.lam = lam;
    HIP_OK(launch_center_offsets(a, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_center_stats(mdbn_ctx* ctx, void* stream, float* stats, int64_t V, int64_t H, int64_t ldv, int64_t ldh, const float* mu,
                      const float* lam, float row_scale, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && stats && mu && lam && workspace, "null pointer");
    REQUIRE(V > 0 && H > 0 && V <= (1 << 30), "sizes must be positive (and V <= 2^30)");
    REQUIRE(H <= CENTER_MAX_H, "H = %lld: at most %d hidden units", (long long)H, CENTER_MAX_H);
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
    REQUIRE(aligned16(stats) && aligned16(workspace), "stats and workspace must be 16-byte aligned");
    REQUIRE((reinterpret_cast<uintptr_t>(mu) & 3u) == 0 && (reinterpret_cast<uintptr_t>(lam) & 3u) == 0, "mu / lam not aligned");
    REQUIRE(row_scale > 0.f && row_scale <= 3.0e38f, "row_scale must be positive and finite");
    REQUIRE(workspace_bytes >= center_partial_floats(V, H) * (int64_t)sizeof(float), "workspace of mdbn_center_workspace_bytes needed");
    CenterStatsArgs a;
    a.stats = stats; a.ldv = ldv; a.ldh = ldh; a.V = (int)V; a.H = (int)H;
    a.rows = center_rows_per_block(V); a.blocks = (int)center_blocks(V); a.ldp = (int)ru4(H);
    a.rho = row_scale; a.mu = mu; a.lam = lam; a.partial = reinterpret_cast<float*>(workspace);
    HIP_OK(launch_center_stats(a, (hipStream_t)stream));
    return MDBN_OK;
}

// ---------------------------------------------------------------------------------- sparsity target (mdbn_sparsity.hip)
int mdbn_sparsity_activity(mdbn_ctx* ctx, void* stream, const float* ph, int64_t ldh, const float* v0, int64_t ldv, int64_t B,
                           int64_t V, int64_t H, float rate, float* q, float* v_mean)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && ph && q, "null pointer");
    REQUIRE((v0 != nullptr) == (v_mean != nullptr), "v0 and v_mean: both or neither");
    REQUIRE(B > 0 && H > 0 && B <= (1 << 30) && H <= (1 << 30), "sizes must be positive (and <= 2^30)");
    REQUIRE(ldh >= H && ldh % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
    REQUIRE(aligned16(ph) && (reinterpret_cast<uintptr_t>(q) & 3u) == 0, "ph must be 16-byte aligned, q float-aligned");
    if (v0) {
        REQUIRE(V > 0 && V <= (1 << 30), "sizes must be positive (and <= 2^30)");
        REQUIRE(ldv >= V && ldv % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
        REQUIRE(aligned16(v0) && (reinterpret_cast<uintptr_t>(v_mean) & 3u) == 0, "v0 must be 16-byte aligned, v_mean float-aligned");
    }
    REQUIRE(rate > 0.f && rate <= 1.f, "rate must lie in (0, 1]");
    SparsityActivityArgs a;
    a.ph = ph; a.v0 = v0; a.ldh = ldh; a.ldv = v0 ? ldv : 0; a.B = (int)B; a.V = v0 ? (int)V : 0; a.H = (int)H;
    a.rate = rate; a.q = q; a.v_mean = v_mean;
    HIP_OK(launch_sparsity_activity(a, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_sparsity_stats(mdbn_ctx* ctx, void* stream, float* stats, int64_t V, int64_t H, int64_t ldv, int64_t ldh, const float* q,
                        const float* v_mean, float target, float w_scale, float b_scale)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && stats && q, "null pointer");
    REQUIRE(V > 0 && H > 0 && V <= (1 << 30) && H <= (1 << 30), "sizes must be positive (and <= 2^30)");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
    REQUIRE(aligned16(stats), "stats must be 16-byte aligned");
    REQUIRE((reinterpret_cast<uintptr_t>(q) & 3u) == 0 && (reinterpret_cast<uintptr_t>(v_mean) & 3u) == 0, "q / v_mean not aligned");
    REQUIRE(target > 0.f && target < 1.f, "target must lie in (0, 1)");
    REQUIRE(w_scale >= 0.f && w_scale <= 3.0e38f && b_scale >= 0.f && b_scale <= 3.0e38f, "scales must be finite and not negative");
    REQUIRE(w_scale == 0.f || v_mean, "w_scale > 0 needs v_mean");
    SparsityStatsArgs a;
    a.stats = stats; a.ldh = ldh; a.V = (int)V; a.H = (int)H; a.rows = center_rows_per_block(V);
    a.q = q; a.v_mean = v_mean; a.target = target; a.w_scale = w_scale; a.b_scale = b_scale;
    HIP_OK(launch_sparsity_stats(a, (hipStream_t)stream));
    return MDBN_OK;
}

// ---------------------------------------------------------------------------------- up-down fine-tuning (mdbn_updown.hip)
}  // extern "C"

// (shared with the grouped generative rule of mdbn_drv_groups.hip through mdbn_capi_internal.h: UpdownWs is declared there)
namespace mdbn {
namespace capi {

bool updown_gen_fused_ok(const mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, UpdownGeom& ug)
{
    return updown_geom(n, V, H, ldv, ldh, std::min(ctx->num_cu, kTargetJobs), ug);
}

bool updown_rec_fused_ok(const mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, ThinGeom& tg)
{
    return thin_geom(n, V, H, ldv, ldh, std::min(ctx->num_cu, kTargetJobs), tg);
}

int updown_inner_floats(int64_t n, int64_t V, int64_t H, int64_t* out)
{
    int64_t bytes = 0;
    CHECK(mdbn_workspace_bytes(n, V, H, &bytes));
    // (a propagation carves a fixed cost region off the end and chunks its rows over what is left: the 8 MB floor of
    //  HipEngine.workspace)
    *out = ru64(std::max<int64_t>((bytes + 3) / 4, int64_t(2) << 20));
    return MDBN_OK;
}

// gen: fused = the cost partials only; composed = stacked operands, prediction, packed statistics, a throw-away hidden bias
// and speed, cost partials, and the workspace of the launchers it strings together
int updown_gen_ws(bool fused, const UpdownGeom& ug, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, UpdownWs& w)
{
    w = UpdownWs{};
    if (fused) { w.partials = ru64(ug.G); return MDBN_OK; }
    w.V2 = ru64(2 * n * ldv); w.P2 = ru64(2 * n * ldh); w.pre = ru64(n * ldv); w.mean = ru64(n * ldv);
    w.stats = ru64(V * ldh + ldh + ldv + 4); w.junk = ru64(2 * ldh); w.partials = ru64(UD_COST_MAXG);
    return updown_inner_floats(n, V, H, &w.inner);
}

// rec: stacked operands, then fused = [s_h | s_v | cost] of the one-pass update, a throw-away visible bias and speed;
// composed = the packed statistics, the same throw-away vectors and the launchers' workspace
int updown_rec_ws(bool fused, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, UpdownWs& w)
{
    w = UpdownWs{};
    w.V2 = ru64(2 * n * ldv); w.P2 = ru64(2 * n * ldh); w.junk = ru64(2 * ldv); w.partials = 64;
    if (fused) { w.stats = ru64(ldh + ldv + 4); return MDBN_OK; }
    w.stats = ru64(V * ldh + ldh + ldv + 4);
    return updown_inner_floats(n, V, H, &w.inner);
}

int updown_check_shape(const mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path)
{
    REQUIRE(ctx != nullptr, "ctx is NULL");
    REQUIRE(n > 0 && V > 0 && H > 0 && n <= (1 << 24) && V <= (1 << 24) && H <= (1 << 24), "sizes must be positive (and <= 2^24)");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
    REQUIRE(path >= 0 && path <= 2, "path must be 0 (by shape), 1 (one-pass kernel) or 2 (composed)");
    return MDBN_OK;
}

// the rule's own arguments: one statement for both halves (stats is ignored; `gen`: the visible half is updated, else the hidden)
int updown_check_update(const mdbn_update_args* u, bool gen)
{
    REQUIRE(u != nullptr, "upd is NULL");
    REQUIRE(u->struct_size == sizeof(mdbn_update_args), "mdbn_update_args.struct_size is %llu, this library's struct has %llu bytes",
            (unsigned long long)u->struct_size, (unsigned long long)sizeof(mdbn_update_args));
    REQUIRE(u->V > 0 && u->H > 0 && u->ldh >= u->H && u->ldv >= u->V && u->ldh % 4 == 0 && u->ldv % 4 == 0, "bad shape / leading dims");
    CHECK(check_mat(u->W, u->ldh, u->H, "W"));
    CHECK(check_mat(u->W_speed, u->ldh, u->H, "W_speed"));
    REQUIRE(u->W0 == nullptr || aligned16(u->W0), "W0 not aligned");
    REQUIRE(u->W_planes == nullptr || aligned16(u->W_planes), "W_planes not aligned");
    if (gen) REQUIRE(u->vbias && u->vbias_speed && !u->hbias && !u->hbias_speed, "generative half: vbias and its speed, hbias NULL");
    else REQUIRE(u->hbias && u->hbias_speed && !u->vbias && !u->vbias_speed, "recognition half: hbias and its speed, vbias NULL");
    REQUIRE(u->batch_size > 0.f && u->n_rows > 0.f, "bad divisors");
    REQUIRE(u->phase == 0, "the delta rules apply the whole rule (phase 0)");
    return MDBN_OK;
}

float* updown_take(float*& p, int64_t floats) { float* r = p; p += floats; return r; }

}  // namespace capi
}  // namespace mdbn

extern "C" {

int mdbn_updown_gen_workspace_bytes(mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    CHECK(updown_check_shape(ctx, n, V, H, ldv, ldh, path));
    UpdownGeom ug{};
    const bool ok = updown_gen_fused_ok(ctx, n, V, H, ldv, ldh, ug);
    REQUIRE(path != 1 || ok, "the one-pass generative kernel serves n <= %d rows on ldh <= %d", UD_MAXB, UD_MAX_LDH);
    UpdownWs w;
    CHECK(updown_gen_ws(path != 2 && ok, ug, n, V, H, ldv, ldh, w));
    *bytes = w.total() * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_updown_gen_step(mdbn_ctx* ctx, void* stream, const float* x_lo, const float* x_hi, int64_t n, int gauss,
                         const mdbn_update_args* upd, float* cost_out, int path, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    CHECK(updown_check_update(upd, true));
    const int64_t V = upd->V, H = upd->H, ldv = upd->ldv, ldh = upd->ldh;
    CHECK(updown_check_shape(ctx, n, V, H, ldv, ldh, path));
    CHECK(check_mat(x_lo, ldv, V, "x_lo"));
    CHECK(check_mat(x_hi, ldh, H, "x_hi"));
    REQUIRE(gauss == 0 || gauss == 1, "gauss must be 0 or 1");
    REQUIRE(cost_out == nullptr || (reinterpret_cast<uintptr_t>(cost_out) & 3u) == 0, "cost_out not aligned");
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    UpdownGeom ug{};
    const bool ok = updown_gen_fused_ok(ctx, n, V, H, ldv, ldh, ug);
    REQUIRE(path != 1 || ok, "the one-pass generative kernel serves n <= %d rows on ldh <= %d", UD_MAXB, UD_MAX_LDH);
    const bool fused = path != 2 && ok;
    UpdownWs w;
    CHECK(updown_gen_ws(fused, ug, n, V, H, ldv, ldh, w));
    REQUIRE(workspace_bytes >= w.total() * (int64_t)sizeof(float), "workspace of mdbn_updown_gen_workspace_bytes needed");
    hipStream_t s = (hipStream_t)stream;
    float* p = reinterpret_cast<float*>(workspace);
    const float scale = upd->cost_scale;

    if (fused) {
        UpdownGenArgs a{};
        a.n = (int)n; a.Bq = ug.Bq; a.V = (int)V; a.H = (int)H; a.ldv = ldv; a.ldh = ldh; a.rpw = ug.rpw; a.G = ug.G;
        a.x_lo = x_lo; a.x_hi = x_hi; a.gauss = gauss;
        fill_upd(a.upd, *upd, V, ldh, reinterpret_cast<unsigned short*>(upd->W_planes));
        a.vb = upd->vbias; a.vbs = upd->vbias_speed; a.inv_rows = 1.0f / upd->n_rows;
        a.cost_partials = p;
        HIP_OK(launch_updown_gen(a, ug, s));
        if (cost_out) HIP_OK(launch_updown_cost_finish(p, ug.G, scale, cost_out, s));
        return MDBN_OK;
    }

    float* V2 = updown_take(p, w.V2); float* P2 = updown_take(p, w.P2);
    float* pre = updown_take(p, w.pre); float* mean = updown_take(p, w.mean);
    float* stats = updown_take(p, w.stats); float* junk = updown_take(p, w.junk);
    float* partials = updown_take(p, w.partials);
    void* inner = p;
    const int64_t inner_bytes = w.inner * (int64_t)sizeof(float);
    // g = act(x_hi G^T + c) with the pre-step parameters
    CHECK(mdbn_propdown_sample(ctx, stream, x_hi, n, ldh, upd->W, V, H, ldv, upd->vbias, gauss, 0, gauss ? nullptr : pre, mean,
                               nullptr, nullptr, nullptr, nullptr, inner, inner_bytes));
    if (cost_out) {
        UpdownCostArgs c{};
        c.n = (int)n; c.V = (int)V; c.gauss = gauss; c.ldv = ldv; c.x = x_lo; c.pre = gauss ? mean : pre;
        c.G = (int)std::min<int64_t>(UD_COST_MAXG, (n * V + UD_COST_NT - 1) / UD_COST_NT);
        c.cost_partials = partials;
        HIP_OK(launch_updown_cost(c, s));
        HIP_OK(launch_updown_cost_finish(partials, c.G, scale, cost_out, s));
    }
    // V2 = [x_lo; g], P2 = [x_hi; -x_hi]: S = (x_lo - g)^T x_hi, s_v = sum (x_lo - g)
    UpdownStackArgs k{};
    k.n = (int)n; k.V = (int)V; k.H = (int)H; k.ldv = ldv; k.ldh = ldh;
    k.lo = x_lo; k.second = mean; k.hi = x_hi; k.neg = x_hi; k.V2 = V2; k.P2 = P2;
    HIP_OK(launch_updown_stack(k, s));
    CHECK(mdbn_cd_stats(ctx, stream, V2, P2, n, V, H, ldv, ldh, stats, inner, inner_bytes));
    mdbn_update_args u = *upd;
    u.stats = stats; u.hbias = junk; u.hbias_speed = junk + ldh; u.cost_out = nullptr;      // the hidden half must not move
    CHECK(mdbn_apply_update(ctx, stream, &u));
    return MDBN_OK;
}

int mdbn_updown_rec_workspace_bytes(mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    CHECK(updown_check_shape(ctx, n, V, H, ldv, ldh, path));
    ThinGeom tg{};
    const bool ok = updown_rec_fused_ok(ctx, n, V, H, ldv, ldh, tg);
    REQUIRE(path != 1 || ok, "the one-pass update serves n <= %d rows on ldh <= 512", TH_MAXB);
    UpdownWs w;
    CHECK(updown_rec_ws(path != 2 && ok, n, V, H, ldv, ldh, w));
    *bytes = w.total() * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_updown_rec_step(mdbn_ctx* ctx, void* stream, const float* y_lo, const float* y_hi, const float* r, int64_t n,
                         const mdbn_update_args* upd, int path, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    CHECK(updown_check_update(upd, false));
    const int64_t V = upd->V, H = upd->H, ldv = upd->ldv, ldh = upd->ldh;
    CHECK(updown_check_shape(ctx, n, V, H, ldv, ldh, path));
    CHECK(check_mat(y_lo, ldv, V, "y_lo"));
    CHECK(check_mat(y_hi, ldh, H, "y_hi"));
    CHECK(check_mat(r, ldh, H, "r"));
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    ThinGeom tg{};
    const bool ok = updown_rec_fused_ok(ctx, n, V, H, ldv, ldh, tg);
    REQUIRE(path != 1 || ok, "the one-pass update serves n <= %d rows on ldh <= 512", TH_MAXB);
    const bool fused = path != 2 && ok;
    UpdownWs w;
    CHECK(updown_rec_ws(fused, n, V, H, ldv, ldh, w));
    REQUIRE(workspace_bytes >= w.total() * (int64_t)sizeof(float), "workspace of mdbn_updown_rec_workspace_bytes needed");
    hipStream_t s = (hipStream_t)stream;
    float* p = reinterpret_cast<float*>(workspace);
    float* V2 = updown_take(p, w.V2); float* P2 = updown_take(p, w.P2);
    float* stats = updown_take(p, w.stats); float* junk = updown_take(p, w.junk);
    float* partials = updown_take(p, w.partials);
    // V2 = [y_lo; y_lo], P2 = [y_hi; -r]: S = y_lo^T (y_hi - r), s_h = sum (y_hi - r)
    UpdownStackArgs k{};
    k.n = (int)n; k.V = (int)V; k.H = (int)H; k.ldv = ldv; k.ldh = ldh;
    k.lo = y_lo; k.second = y_lo; k.hi = y_hi; k.neg = r; k.V2 = V2; k.P2 = P2;
    HIP_OK(launch_updown_stack(k, s));
    mdbn_update_args u = *upd;
    u.vbias = junk; u.vbias_speed = junk + ldv; u.cost_out = nullptr;                       // the visible half must not move
    if (fused) {
        // the rank-2n update of thin_update_kernel on the stacked operands: W and its speed read and written once
        ThinUpdArgs t{};
        t.B = (int)n; t.Bq = tg.Bq; t.V = (int)V; t.H = (int)H; t.ldv = ldv; t.ldh = ldh; t.G = tg.Gu; t.rpw = tg.rpu;
        t.V2 = V2; t.P2 = P2;
        t.S = nullptr; t.s_h = stats; t.s_v = stats + ldh; t.cost = stats + ldh + ldv;
        t.cost_partials = partials; t.n_cost = 0;
        t.do_upd = 1;
        fill_upd(t.upd, u, V, ldh, reinterpret_cast<unsigned short*>(u.W_planes));
        fill_bias_upd(t.bu, u, H);
        HIP_OK(launch_thin_update(t, tg, s));
        return MDBN_OK;
    }
    void* inner = p;
    const int64_t inner_bytes = w.inner * (int64_t)sizeof(float);
    CHECK(mdbn_cd_stats(ctx, stream, V2, P2, n, V, H, ldv, ldh, stats, inner, inner_bytes));
    u.stats = stats;
    CHECK(mdbn_apply_update(ctx, stream, &u));
    return MDBN_OK;
}

}  // extern "C"

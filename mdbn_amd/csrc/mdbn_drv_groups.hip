// C-ABI drivers of the categorical visible units (declared in include/mdbn_hip.h): the grouped softmax kernel alone
// (mdbn_groups.hip), the CD step of a layer with groups, composed from the propagation passes of the core, that kernel and
// mdbn_cd_stats, and the generative delta rule of up-down fine-tuning on such a layer (mdbn_updown.hip: the one-pass kernel, or
// the composed path of the plain rule with the grouped means).  Of the core they use what mdbn_capi_internal.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "mdbn_capi_internal.h"
#include "mdbn_groups.h"
#include "mdbn_updown.h"

using namespace mdbn;
using namespace mdbn::capi;

// The table as the host holds it: strictly ascending boundaries inside [0, V], every group of 2 .. MDBN_GROUP_MAX columns.
// n_groups = 0: no table is read (both pointers may be NULL).  -> the span [lo, hi) the groups cover
int mdbn::capi::check_groups(const int32_t* dev, const int32_t* host, int64_t n_groups, int64_t V, int& lo, int& hi)
{
    REQUIRE(n_groups >= 0 && n_groups <= V / 2, "n_groups = %lld: between 0 and V / 2", (long long)n_groups);
    lo = hi = (int)V;
    if (n_groups == 0) return MDBN_OK;
    REQUIRE(dev != nullptr && host != nullptr, "group_start: the device and the host copy are both needed");
    REQUIRE((reinterpret_cast<uintptr_t>(dev) & 3u) == 0 && (reinterpret_cast<uintptr_t>(host) & 3u) == 0, "group_start not aligned");
    REQUIRE(host[0] >= 0 && host[n_groups] <= V, "group table: boundaries %d .. %d leave the %lld visible units", host[0],
            host[n_groups], (long long)V);
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t K = (int64_t)host[g + 1] - host[g];
        REQUIRE(K >= 2 && K <= MDBN_GROUP_MAX, "group %lld has %lld columns: 2 .. %d (boundaries strictly ascending)", (long long)g,
                (long long)K, MDBN_GROUP_MAX);
    }
    lo = host[0]; hi = host[n_groups];
    return MDBN_OK;
}

namespace {

int64_t group_partial_floats(int64_t B, int64_t V) { return ru64(group_softmax_blocks(B, V)); }    // (units <= V)

// the generative delta rule of a layer with groups: the one-pass kernel's regime is that of the plain rule (updown_geom)
bool updown_gen_grouped_fused_ok(const mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, UpdownGeom& ug)
{
    return updown_geom_grouped(n, V, H, ldv, ldh, std::min(ctx->num_cu, kTargetJobs), ug);
}

// ... and its workspace that of the plain rule, the composed path's cost partials those of the grouped softmax launch
int updown_gen_grouped_ws(bool fused, const UpdownGeom& ug, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, UpdownWs& w)
{
    CHECK(updown_gen_ws(fused, ug, n, V, H, ldv, ldh, w));
    if (fused) return MDBN_OK;
    REQUIRE(group_softmax_blocks(n, V) <= 0x7fffffff, "n = %lld rows of V = %lld units: too many for one grouped softmax launch",
            (long long)n, (long long)V);
    w.partials = std::max(w.partials, group_partial_floats(n, V));
    return MDBN_OK;
}

}  // namespace

extern "C" {

int mdbn_group_softmax_workspace_bytes(mdbn_ctx* ctx, int64_t B, int64_t V, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && bytes && B > 0 && V > 0 && B <= (1 << 24) && V <= (1 << 24), "bad arguments (0 < B, V <= 2^24)");
    *bytes = group_partial_floats(B, V) * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_group_softmax_sample(mdbn_ctx* ctx, void* stream, const float* pre, int64_t B, int64_t ldv, int64_t V,
                              const int32_t* group_start, const int32_t* group_start_host, int64_t n_groups, float* mean,
                              float* sample, float* tap, const mdbn_rng* rng, const float* v0, float* cost_sum, void* workspace,
                              int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr, "ctx is NULL");
    REQUIRE(B > 0 && V > 0 && B <= (1 << 24) && V <= (1 << 24), "sizes must be positive (and <= 2^24)");
    CHECK(check_mat(pre, ldv, V, "pre"));
    for (const float* p : {(const float*)mean, (const float*)sample, (const float*)tap, v0})
        REQUIRE(p == nullptr || aligned16(p), "mean / sample / tap / v0 not 16-byte aligned");
    REQUIRE((sample == nullptr && tap == nullptr) || rng != nullptr, "sampling needs rng");
    REQUIRE((v0 == nullptr) == (cost_sum == nullptr), "v0 and cost_sum go together");
    REQUIRE(cost_sum == nullptr || aligned16(cost_sum), "cost_sum (4 floats) not 16-byte aligned");
    int lo, hi;
    CHECK(check_groups(group_start, group_start_host, n_groups, V, lo, hi));
    if (v0) {
        REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
        REQUIRE(workspace_bytes >= group_partial_floats(B, V) * (int64_t)sizeof(float), "workspace of mdbn_group_softmax_workspace_bytes needed");
    }
    GroupSoftmaxArgs g{};
    g.pre = pre; g.mean = mean; g.sample = sample; g.tap = tap; g.v0 = v0;
    g.cost_partials = v0 ? reinterpret_cast<float*>(workspace) : nullptr;
    g.group_start = group_start; g.n_groups = (int)n_groups; g.span_lo = lo; g.span_hi = hi;
    g.B = (int)B; g.V = (int)V; g.units = group_units((int)V, lo, hi, (int)n_groups); g.ld = ldv;
    mdbn_rng zero{};
    g.rng = make_key(rng ? *rng : zero, rng ? rng->draw : 0u);
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(launch_group_softmax(g, s));
    if (cost_sum)
        HIP_OK(launch_finalize_stats(nullptr, nullptr, nullptr, 0, 0, 0, g.cost_partials, (int)group_softmax_blocks(B, g.units), nullptr,
                                     nullptr, cost_sum, nullptr, s));
    return MDBN_OK;
}

int mdbn_center_hidden_rows(mdbn_ctx* ctx, void* stream, const float* V2, int64_t ldv, const float* P2, int64_t ldh, int64_t B,
                            int64_t V, int64_t H, const float* stats, const float* mu, const float* lam, float row_scale,
                            const float* q, const float* v_mean, float target, float w_scale, float b_scale, float* s_h_out,
                            void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && V2 && P2 && stats && mu && lam && s_h_out && workspace, "null pointer");
    REQUIRE(B > 0 && V > 0 && H > 0 && B <= (1 << 24) && V <= (1 << 24) && H <= (1 << 24), "sizes must be positive (and <= 2^24)");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dimensions: ld >= cols, ld %% 4 == 0");
    REQUIRE(aligned16(V2) && aligned16(P2) && aligned16(stats), "V2, P2 and stats must be 16-byte aligned");
    for (const void* p : {(const void*)mu, (const void*)lam, (const void*)s_h_out, (const void*)workspace})
        REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, "mu / lam / s_h_out / workspace not aligned");
    REQUIRE(row_scale > 0.f && row_scale <= 3.0e38f, "row_scale must be positive and finite");
    REQUIRE(workspace_bytes >= (2 * B + 3) * (int64_t)sizeof(float), "workspace of (2 B + 3) floats needed");
    if (q) {
        REQUIRE((reinterpret_cast<uintptr_t>(q) & 3u) == 0 && (reinterpret_cast<uintptr_t>(v_mean) & 3u) == 0, "q / v_mean not aligned");
        REQUIRE(target > 0.f && target < 1.f, "target must lie in (0, 1)");
        REQUIRE(w_scale >= 0.f && w_scale <= 3.0e38f && b_scale >= 0.f && b_scale <= 3.0e38f, "scales must be finite and not negative");
        REQUIRE(w_scale == 0.f || v_mean, "w_scale > 0 needs v_mean");
    }
    CenterHiddenArgs a{};
    a.q = q; a.v_mean = (q && w_scale != 0.f) ? v_mean : nullptr; a.target = target; a.w_scale = q ? w_scale : 0.f; a.b_scale = q ? b_scale : 0.f;
    a.V2 = V2; a.P2 = P2; a.stats = stats; a.mu = mu; a.lam = lam; a.d = reinterpret_cast<float*>(workspace); a.out = s_h_out;
    a.ldv = ldv; a.ldh = ldh; a.B = (int)B; a.V = (int)V; a.H = (int)H; a.rho = row_scale;
    HIP_OK(launch_center_hidden(a, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_cd_step_grouped(mdbn_ctx* ctx, void* stream, const mdbn_cd_args* a, const int32_t* group_start,
                         const int32_t* group_start_host, int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr && a != nullptr, "NULL argument");
    REQUIRE(a->struct_size == sizeof(mdbn_cd_args),
            "mdbn_cd_args.struct_size is %llu, this library's struct has %llu bytes (built against another mdbn_hip.h?)",
            (unsigned long long)a->struct_size, (unsigned long long)sizeof(mdbn_cd_args));
    const int64_t B = a->B, V = a->V, H = a->H, ldv = a->ldv, ldh = a->ldh;
    REQUIRE(B > 0 && V > 0 && H > 0 && a->k >= 1 && B <= (1 << 24) && V <= (1 << 24), "bad shape / k");
    REQUIRE(!a->gauss, "categorical visible units: a Gaussian layer (gauss = 1) has no groups");
    REQUIRE(!a->sample_stats, "categorical visible units: sample_stats is not supported");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dims must be multiples of 4, >= V / H");
    CHECK(check_mat(a->data, ldv, V, "data"));
    CHECK(check_mat(a->W, ldh, H, "W"));
    CHECK(check_mat(a->V2, ldv, V, "V2"));
    CHECK(check_mat(a->P2, ldh, H, "P2"));
    CHECK(check_mat(a->hs, ldh, H, "hs"));
    CHECK(check_mat(a->vs, ldv, V, "vs"));
    REQUIRE(a->hbias && a->vbias, "bias pointers are NULL");
    REQUIRE(a->stats != nullptr && aligned16(a->stats), "stats not aligned");
    REQUIRE(a->persistent == nullptr || aligned16(a->persistent), "persistent not aligned");
    REQUIRE(a->indexes != nullptr || B <= a->n_data, "identity minibatch longer than data");
    int lo, hi;
    CHECK(check_groups(group_start, group_start_host, n_groups, V, lo, hi));
    Workspace probe;                                   // the statistics' carve-up is the largest: refused here, before any launch
    CHECK(carve(a->workspace, a->workspace_bytes, B, V, H, probe, true, ldv, ldh));
    REQUIRE(a->workspace_bytes >= group_partial_floats(B, V) * (int64_t)sizeof(float), "workspace too small for the cost partials");
    Workspace ws;
    CHECK(carve(a->workspace, a->workspace_bytes, B, V, H, ws, false));
    hipStream_t s = (hipStream_t)stream;
    float *v0 = a->V2, *nv = a->V2 + B * ldv, *ph = a->P2, *nh = a->P2 + B * ldh;
    float* cost = a->stats + V * ldh + ldh + ldv;

    HIP_OK(launch_gather(a->data, a->n_data, ldv, ldv, a->indexes, a->index_is_64, B, v0, ldv, s));
    // the kernel leaves pad columns alone; the propup that reads vs wants them zero
    if (ldv > V) HIP_OK(hipMemset2DAsync(a->vs + V, sizeof(float) * ldv, 0, sizeof(float) * (ldv - V), B, s));
    {                                                                   // positive phase: draw 0
        Affine up(v0, B, ldv, a->W, V, H, ldh, a->hbias);
        up.mean = ph; up.sample = a->hs; up.rng = &a->rng;
        CHECK(run_affine(up, ws, s, nullptr));
        if (a->trace_h) HIP_OK(hipMemcpyAsync(a->trace_h, a->hs, sizeof(float) * B * ldh, hipMemcpyDeviceToDevice, s));
    }
    GroupSoftmaxArgs g{};
    g.group_start = group_start; g.n_groups = (int)n_groups; g.span_lo = lo; g.span_hi = hi;
    g.B = (int)B; g.V = (int)V; g.units = group_units((int)V, lo, hi, (int)n_groups); g.ld = ldv;
    for (int t = 1; t <= a->k; ++t) {                                   // gibbs_hvh x k: draws 2t - 1 (visible), 2t (hidden)
        const bool last = t == a->k;
        const float* chain = (t == 1 && a->persistent) ? a->persistent : a->hs;
        // the linear pre-activations h W^T + vbias into rows B.. of V2, then the kernel turns them into means in place
        Affine down(chain, B, ldh, a->W, V, H, ldh, a->vbias, ldv, 1);
        down.mean = nv;
        down.x_binary = chain == a->hs;
        CHECK(run_affine(down, ws, s, nullptr));
        g.pre = nv; g.mean = nv; g.sample = a->vs;
        g.tap = a->trace_v ? a->trace_v + (int64_t)(t - 1) * B * ldv : nullptr;
        g.v0 = last ? v0 : nullptr;
        g.cost_partials = last ? reinterpret_cast<float*>(a->workspace) : nullptr;    // (consumed before the next pass's slabs)
        g.rng = make_key(a->rng, (uint32_t)(2 * t - 1));
        HIP_OK(launch_group_softmax(g, s));
        if (last)
            HIP_OK(launch_finalize_stats(nullptr, nullptr, nullptr, 0, 0, 0, g.cost_partials, (int)group_softmax_blocks(B, g.units),
                                         nullptr, nullptr, cost, nullptr, s));
        const bool need_sample = !last || a->persistent != nullptr;
        float* hdst = (last && a->persistent) ? a->persistent : a->hs;
        Affine up(a->vs, B, ldv, a->W, V, H, ldh, a->hbias);
        up.mean = nh; up.sample = need_sample ? hdst : nullptr; up.mean_scale = -1.0f;
        up.rng = &a->rng; up.draw = (uint32_t)(2 * t);
        up.x_binary = true;
        CHECK(run_affine(up, ws, s, nullptr));
        if (a->trace_h && need_sample)
            HIP_OK(hipMemcpyAsync(a->trace_h + (int64_t)t * B * ldh, hdst, sizeof(float) * B * ldh, hipMemcpyDeviceToDevice, s));
    }
    return mdbn_cd_stats(ctx, stream, a->V2, a->P2, B, V, H, ldv, ldh, a->stats, a->workspace, a->workspace_bytes);
}

// ---------------------------------------------------------------------------------- up-down fine-tuning, a layer with groups
int mdbn_updown_gen_grouped_workspace_bytes(mdbn_ctx* ctx, int64_t n, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int path,
                                            int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    CHECK(updown_check_shape(ctx, n, V, H, ldv, ldh, path));
    UpdownGeom ug{};
    const bool ok = updown_gen_grouped_fused_ok(ctx, n, V, H, ldv, ldh, ug);
    REQUIRE(path != 1 || ok, "the one-pass generative kernel serves n <= %d rows on ldh <= %d", UD_MAXB, UD_MAX_LDH);
    UpdownWs w;
    CHECK(updown_gen_grouped_ws(path != 2 && ok, ug, n, V, H, ldv, ldh, w));
    *bytes = w.total() * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_updown_gen_step_grouped(mdbn_ctx* ctx, void* stream, const float* x_lo, const float* x_hi, int64_t n,
                                 const mdbn_update_args* upd, float* cost_out, int path, void* workspace, int64_t workspace_bytes,
                                 const int32_t* group_start, const int32_t* group_start_host, int64_t n_groups)
{
    CtxScope ctx_scope(ctx);
    CHECK(updown_check_update(upd, true));
    const int64_t V = upd->V, H = upd->H, ldv = upd->ldv, ldh = upd->ldh;
    CHECK(updown_check_shape(ctx, n, V, H, ldv, ldh, path));
    CHECK(check_mat(x_lo, ldv, V, "x_lo"));
    CHECK(check_mat(x_hi, ldh, H, "x_hi"));
    REQUIRE(cost_out == nullptr || (reinterpret_cast<uintptr_t>(cost_out) & 3u) == 0, "cost_out not aligned");
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    REQUIRE(n_groups >= 1, "n_groups = %lld: a layer without groups takes mdbn_updown_gen_step", (long long)n_groups);
    int lo, hi;
    CHECK(check_groups(group_start, group_start_host, n_groups, V, lo, hi));
    UpdownGeom ug{};
    const bool ok = updown_gen_grouped_fused_ok(ctx, n, V, H, ldv, ldh, ug);
    REQUIRE(path != 1 || ok, "the one-pass generative kernel serves n <= %d rows on ldh <= %d", UD_MAXB, UD_MAX_LDH);
    const bool fused = path != 2 && ok;
    UpdownWs w;
    CHECK(updown_gen_grouped_ws(fused, ug, n, V, H, ldv, ldh, w));
    REQUIRE(workspace_bytes >= w.total() * (int64_t)sizeof(float), "workspace of mdbn_updown_gen_grouped_workspace_bytes needed");
    hipStream_t s = (hipStream_t)stream;
    float* p = reinterpret_cast<float*>(workspace);
    const float scale = upd->cost_scale;

    if (fused) {
        UpdownGenGroupedArgs q{};
        UpdownGenArgs& a = q.g;
        a.n = (int)n; a.Bq = ug.Bq; a.V = (int)V; a.H = (int)H; a.ldv = ldv; a.ldh = ldh; a.rpw = ug.rpw; a.G = ug.G;
        a.x_lo = x_lo; a.x_hi = x_hi; a.gauss = 0;
        fill_upd(a.upd, *upd, V, ldh, reinterpret_cast<unsigned short*>(upd->W_planes));
        a.vb = upd->vbias; a.vbs = upd->vbias_speed; a.inv_rows = 1.0f / upd->n_rows;
        a.cost_partials = p;
        q.group_start = group_start; q.n_groups = (int)n_groups; q.span_lo = lo; q.span_hi = hi;
        HIP_OK(launch_updown_gen_grouped(q, ug, s));
        if (cost_out) HIP_OK(launch_updown_cost_finish(p, ug.G, scale, cost_out, s));
        return MDBN_OK;
    }

    float* V2 = updown_take(p, w.V2); float* P2 = updown_take(p, w.P2);
    updown_take(p, w.pre); float* mean = updown_take(p, w.mean);
    float* stats = updown_take(p, w.stats); float* junk = updown_take(p, w.junk);
    float* partials = updown_take(p, w.partials);
    void* inner = p;
    const int64_t inner_bytes = w.inner * (int64_t)sizeof(float);
    // the linear pre-activations x_hi G^T + c with the pre-step parameters, then the grouped means in place
    CHECK(mdbn_propdown_sample(ctx, stream, x_hi, n, ldh, upd->W, V, H, ldv, upd->vbias, 1, 0, nullptr, mean, nullptr, nullptr,
                               nullptr, nullptr, inner, inner_bytes));
    GroupSoftmaxArgs g{};
    g.pre = mean; g.mean = mean; g.v0 = cost_out ? x_lo : nullptr; g.cost_partials = cost_out ? partials : nullptr;
    g.group_start = group_start; g.n_groups = (int)n_groups; g.span_lo = lo; g.span_hi = hi;
    g.B = (int)n; g.V = (int)V; g.units = group_units((int)V, lo, hi, (int)n_groups); g.ld = ldv;
    mdbn_rng zero{};
    g.rng = make_key(zero, 0u);
    HIP_OK(launch_group_softmax(g, s));
    if (cost_out) HIP_OK(launch_updown_cost_finish(partials, (int)group_softmax_blocks(n, g.units), scale, cost_out, s));
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

}  // extern "C"

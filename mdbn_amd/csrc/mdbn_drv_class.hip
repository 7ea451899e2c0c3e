// C-ABI drivers of the classification RBM (declared in include/mdbn_hip.h): the posterior of a label block from one propup and
// the class kernel (mdbn_class.hip), and the discriminative / hybrid statistics -- the class kernel's operand rows stacked
// beside those of the CD step, ONE mdbn_cd_stats over the stack, then the patch kernel.  Of the core they use what
// mdbn_capi_internal.h declares and the public propup / statistics calls.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "mdbn_capi_internal.h"
#include "mdbn_class.h"

using namespace mdbn;
using namespace mdbn::capi;

namespace {

// rows per batch and workgroups of class_forward: B = 20 still spreads over the CUs (one row each), B = 512 fills them
// (two rows each); training keeps one [K][ldh] partial of T per workgroup, so their number is capped by that memory
constexpr int64_t kClassPartialFloats = int64_t(32) << 20;
struct ClassGeom { int R, G; };
ClassGeom class_geom(const mdbn_ctx* ctx, int64_t B, int64_t K, int64_t ldh, bool train)
{
    const int64_t cu = std::max(ctx->num_cu, 1);
    ClassGeom g;
    g.R = (int)std::min<int64_t>(CLASS_R, std::max<int64_t>(1, (B + cu - 1) / cu));
    int64_t n = (B + g.R - 1) / g.R;
    if (train) n = std::min(n, std::min<int64_t>(4 * cu, std::max<int64_t>(1, kClassPartialFloats / (K * ldh))));
    g.G = (int)n;
    return g;
}

// the workspace in floats, every piece a multiple of 64 floats; `inner`: what the propup and mdbn_cd_stats are handed
struct ClassWs {
    int64_t V2s = 0, P2s = 0, pre = 0, Tp = 0, np = 0, nllp = 0, svp = 0, inner = 0;
    int64_t total() const { return V2s + P2s + pre + Tp + np + nllp + svp + inner; }
};

int class_ws(const mdbn_ctx* ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t K, int mode, ClassWs& w)
{
    w = ClassWs{};
    int64_t up = 0, st = 0;
    CHECK(mdbn_workspace_bytes(B, V, H, &up));
    w.pre = ru64(B * ldh);
    if (mode == MDBN_CLASS_POSTERIOR) {
        w.V2s = ru64(B * ldv);
    } else {
        const int64_t stack = mode == MDBN_CLASS_HYBRID ? 4 * B : 2 * B;       // rows of the stacked operands
        const ClassGeom g = class_geom(ctx, B, K, ldh, true);
        w.V2s = ru64(stack * ldv); w.P2s = ru64(stack * ldh);
        w.Tp = ru64((int64_t)g.G * K * ldh); w.np = ru64((int64_t)g.G * MDBN_GROUP_MAX); w.nllp = ru64(g.G);
        if (mode == MDBN_CLASS_HYBRID) w.svp = ru64((int64_t)class_prep_chunks(B) * ldv);
        CHECK(mdbn_workspace_bytes_ld(stack / 2, V, H, ldv, ldh, &st));
    }
    w.inner = ru64((std::max(up, st) + 3) / 4);
    return MDBN_OK;
}

int class_check_shape(const mdbn_ctx* ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t lo, int64_t K)
{
    REQUIRE(ctx != nullptr, "ctx is NULL");
    REQUIRE(B > 0 && V > 0 && H > 0 && B <= (1 << 24) && V <= (1 << 24) && H <= (1 << 24), "sizes must be positive (and <= 2^24)");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dims must be multiples of 4, >= V / H");
    REQUIRE(K >= 2 && K <= MDBN_GROUP_MAX, "the label block has %lld columns: 2 .. %d", (long long)K, MDBN_GROUP_MAX);
    REQUIRE(lo >= 0 && lo + K <= V, "the label block, columns %lld .. %lld, leaves the %lld visible units", (long long)lo,
            (long long)(lo + K - 1), (long long)V);
    return MDBN_OK;
}

float* take(float*& p, int64_t floats) { float* r = p; p += floats; return r; }

}  // namespace

extern "C" {

int mdbn_class_workspace_bytes(mdbn_ctx* ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t K, int mode,
                               int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(bytes != nullptr, "bytes is NULL");
    REQUIRE(mode == MDBN_CLASS_POSTERIOR || mode == MDBN_CLASS_PURE || mode == MDBN_CLASS_HYBRID, "mode must be 0, 1 or 2");
    CHECK(class_check_shape(ctx, B, V, H, ldv, ldh, 0, K));
    ClassWs w;
    CHECK(class_ws(ctx, B, V, H, ldv, ldh, K, mode, w));
    *bytes = w.total() * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_class_posterior(mdbn_ctx* ctx, void* stream, const float* v, int64_t B, int64_t ldv, const float* W, int64_t V, int64_t H,
                         int64_t ldh, const float* hbias, const float* vbias, int64_t lo, int64_t K, float* post, int64_t ldk,
                         float* logp, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    CHECK(class_check_shape(ctx, B, V, H, ldv, ldh, lo, K));
    CHECK(check_mat(v, ldv, V, "v"));
    CHECK(check_mat(W, ldh, H, "W"));
    REQUIRE(hbias != nullptr && vbias != nullptr, "bias pointers are NULL");
    REQUIRE(post != nullptr && (reinterpret_cast<uintptr_t>(post) & 3u) == 0 && ldk >= K, "post: a float matrix of ldk >= K columns");
    REQUIRE(logp == nullptr || (reinterpret_cast<uintptr_t>(logp) & 3u) == 0, "logp not aligned");
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    ClassWs w;
    CHECK(class_ws(ctx, B, V, H, ldv, ldh, K, MDBN_CLASS_POSTERIOR, w));
    if (workspace_bytes < w.total() * (int64_t)sizeof(float))
        return fail(MDBN_ENOSPC, "workspace of %lld bytes: mdbn_class_workspace_bytes asks for %lld", (long long)workspace_bytes,
                    (long long)(w.total() * (int64_t)sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    float* p = reinterpret_cast<float*>(workspace);
    float* xt = take(p, w.V2s); float* pre = take(p, w.pre);
    void* inner = p;
    const int64_t inner_bytes = w.inner * (int64_t)sizeof(float);

    ClassPrepArgs q{};
    q.v0 = v; q.xt = xt; q.B = (int)B; q.V = (int)V; q.lo = (int)lo; q.K = (int)K; q.ldv = ldv;
    HIP_OK(launch_class_prep(q, s));
    CHECK(mdbn_propup_sample(ctx, stream, xt, B, ldv, W, V, H, ldh, hbias, pre, nullptr, 1.0f, nullptr, nullptr, inner, inner_bytes));
    const ClassGeom geo = class_geom(ctx, B, K, ldh, false);
    ClassForwardArgs f{};
    f.A = pre; f.U = W + lo * ldh; f.d = vbias + lo;
    f.label = logp ? v + lo : nullptr; f.ld_label = ldv;
    f.post = post; f.ldk = ldk; f.logp = logp;
    f.B = (int)B; f.H = (int)H; f.K = (int)K; f.G = geo.G; f.R = geo.R; f.ldh = ldh;
    HIP_OK(launch_class_forward(f, s));
    return MDBN_OK;
}

int mdbn_class_stats(mdbn_ctx* ctx, void* stream, const float* V2, const float* P2, int64_t B, const float* W, int64_t V, int64_t H,
                     int64_t ldv, int64_t ldh, const float* hbias, const float* vbias, int64_t lo, int64_t K, float gen_weight,
                     float disc_weight, float* stats, float* nll_sum, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    CHECK(class_check_shape(ctx, B, V, H, ldv, ldh, lo, K));
    REQUIRE(std::isfinite(gen_weight) && std::isfinite(disc_weight) && gen_weight >= 0.f && disc_weight >= 0.f,
            "gen_weight = %g, disc_weight = %g: finite and not negative", (double)gen_weight, (double)disc_weight);
    REQUIRE(gen_weight > 0.f || disc_weight > 0.f, "gen_weight and disc_weight are both 0: nothing to compute");
    const bool hybrid = gen_weight > 0.f;
    CHECK(check_mat(V2, ldv, V, "V2"));
    CHECK(check_mat(W, ldh, H, "W"));
    if (hybrid) CHECK(check_mat(P2, ldh, H, "P2"));
    REQUIRE(hbias != nullptr && vbias != nullptr, "bias pointers are NULL");
    REQUIRE(stats != nullptr && aligned16(stats), "stats must be 16-byte aligned");
    REQUIRE(nll_sum == nullptr || (reinterpret_cast<uintptr_t>(nll_sum) & 3u) == 0, "nll_sum not aligned");
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    ClassWs w;
    CHECK(class_ws(ctx, B, V, H, ldv, ldh, K, hybrid ? MDBN_CLASS_HYBRID : MDBN_CLASS_PURE, w));
    if (workspace_bytes < w.total() * (int64_t)sizeof(float))
        return fail(MDBN_ENOSPC, "workspace of %lld bytes: mdbn_class_workspace_bytes asks for %lld", (long long)workspace_bytes,
                    (long long)(w.total() * (int64_t)sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    float* p = reinterpret_cast<float*>(workspace);
    float* V2s = take(p, w.V2s); float* P2s = take(p, w.P2s); float* pre = take(p, w.pre);
    float* Tp = take(p, w.Tp); float* np = take(p, w.np); float* nllp = take(p, w.nllp); float* svp = take(p, w.svp);
    void* inner = p;
    const int64_t inner_bytes = w.inner * (int64_t)sizeof(float);
    const int64_t rv = B * ldv, rh = B * ldh;
    // hybrid: V2' = [v0; v0 | nv; x~], P2' = [gen ph; w r_pos | -gen nh; -w r_bar];  pure: V2' = [v0 | x~], P2' = [w r_pos | -w r_bar]
    float* xt = hybrid ? V2s + 3 * rv : V2s + rv;

    ClassPrepArgs q{};
    q.v0 = V2; q.copy0 = V2s; q.xt = xt;
    if (hybrid) { q.nv = V2 + rv; q.copy1 = V2s + rv; q.copy_nv = V2s + 2 * rv; q.svp = svp; }
    q.B = (int)B; q.V = (int)V; q.lo = (int)lo; q.K = (int)K; q.ldv = ldv;
    HIP_OK(launch_class_prep(q, s));
    CHECK(mdbn_propup_sample(ctx, stream, xt, B, ldv, W, V, H, ldh, hbias, pre, nullptr, 1.0f, nullptr, nullptr, inner, inner_bytes));
    const ClassGeom geo = class_geom(ctx, B, K, ldh, true);
    ClassForwardArgs f{};
    f.A = pre; f.U = W + lo * ldh; f.d = vbias + lo;
    f.label = V2 + lo; f.ld_label = ldv;
    if (hybrid) {
        f.ph = P2; f.nh = P2 + rh; f.ph_out = P2s; f.rpos = P2s + rh; f.nh_out = P2s + 2 * rh; f.rbar = P2s + 3 * rh;
    } else {
        f.rpos = P2s; f.rbar = P2s + rh;
    }
    f.Tp = Tp; f.np = np; f.nllp = nllp; f.w = disc_weight; f.gen = gen_weight;
    f.B = (int)B; f.H = (int)H; f.K = (int)K; f.G = geo.G; f.R = geo.R; f.ldh = ldh;
    HIP_OK(launch_class_forward(f, s));
    CHECK(mdbn_cd_stats(ctx, stream, V2s, P2s, hybrid ? 2 * B : B, V, H, ldv, ldh, stats, inner, inner_bytes));
    ClassPatchArgs c{};
    c.Tp = Tp; c.np = np; c.nllp = nllp; c.svp = hybrid ? svp : nullptr;
    c.S = stats; c.s_v = stats + V * ldh + ldh; c.nll_out = nll_sum; c.cost_out = hybrid ? nullptr : stats + V * ldh + ldh + ldv;
    c.w = disc_weight; c.gen = gen_weight;
    c.V = (int)V; c.H = (int)H; c.K = (int)K; c.lo = (int)lo; c.G = geo.G; c.chunks = class_prep_chunks(B); c.ldv = ldv; c.ldh = ldh;
    HIP_OK(launch_class_patch(c, s));
    return MDBN_OK;
}

}  // extern "C"

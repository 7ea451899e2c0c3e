// C-ABI drivers of the absent visible units (declared in include/mdbn_hip.h): the row kernels of mdbn_absent.hip alone, the CD
// step on rows with missing entries -- mdbn_cd_step_grouped's composition from the propagation passes of the core, the masked
// visible kernel and mdbn_cd_stats --, and the free energy over the observed units.  Of the core they use what
// mdbn_capi_internal.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "mdbn_capi_internal.h"
#include "mdbn_absent.h"

using namespace mdbn;
using namespace mdbn::capi;

namespace {

constexpr int64_t kF = (int64_t)sizeof(float);

int64_t mask_floats(int64_t B, int64_t V) { return ru64(B * absent_words(V)); }           // (uint32 words: 4 bytes each)
int64_t partial_floats(int64_t B, int64_t V) { return ru64(absent_visible_blocks(B, V)); }

int check_shape(int64_t B, int64_t V)
{
    REQUIRE(B > 0 && V > 0 && B <= (1 << 24) && V <= (1 << 24), "sizes must be positive (and <= 2^24)");
    REQUIRE(absent_split_blocks(B, V) <= 0x7fffffff, "B = %lld rows of V = %lld units: too many for one launch", (long long)B, (long long)V);
    return MDBN_OK;
}

// the carve-up of mdbn_cd_step_absent: [the step's own workspace | mask words | cost partials]
int step_dense_bytes(int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t& dense)
{
    CHECK(mdbn_workspace_bytes_ld(B, V, H, ldv, ldh, &dense));
    dense = ru64(dense / kF + (dense % kF != 0)) * kF;
    return MDBN_OK;
}

// ... and of mdbn_free_energy_absent: [zero-filled rows | mask words | the workspace of mdbn_free_energy]
int fe_inner_bytes(int64_t N, int64_t V, int64_t H, int64_t& inner)
{
    return mdbn_workspace_bytes(std::min<int64_t>(N, 4096), V, H, &inner);
}

}  // namespace

extern "C" {

int mdbn_absent_split(mdbn_ctx* ctx, void* stream, const float* x, int64_t B, int64_t ldx, int64_t V, float* filled,
                      int64_t ld_filled, uint32_t* observed, int32_t* row_count)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr, "ctx is NULL");
    CHECK(check_shape(B, V));
    CHECK(check_mat(x, ldx, V, "x"));
    CHECK(check_mat(filled, ld_filled, V, "filled"));
    REQUIRE(observed != nullptr && (reinterpret_cast<uintptr_t>(observed) & 3u) == 0, "observed is NULL or not aligned");
    REQUIRE((reinterpret_cast<uintptr_t>(row_count) & 3u) == 0, "row_count not aligned");
    AbsentSplitArgs a{};
    a.x = x; a.ldx = ldx; a.filled = filled; a.ld_filled = ld_filled; a.observed = observed; a.row_count = row_count;
    a.B = (int)B; a.V = (int)V;
    HIP_OK(launch_absent_split(a, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_absent_visible_workspace_bytes(mdbn_ctx* ctx, int64_t B, int64_t V, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr && bytes != nullptr, "NULL argument");
    CHECK(check_shape(B, V));
    *bytes = partial_floats(B, V) * kF;
    return MDBN_OK;
}

int mdbn_absent_visible(mdbn_ctx* ctx, void* stream, const float* pre, int64_t B, int64_t ldv, int64_t V, const uint32_t* observed,
                        int gauss, int add_noise, float* mean, float* sample, float* tap, const mdbn_rng* rng, const float* v0,
                        float* cost_sum, void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr, "ctx is NULL");
    CHECK(check_shape(B, V));
    CHECK(check_mat(pre, ldv, V, "pre"));
    REQUIRE(observed != nullptr && (reinterpret_cast<uintptr_t>(observed) & 3u) == 0, "observed is NULL or not aligned");
    for (const float* p : {(const float*)mean, (const float*)sample, (const float*)tap, v0})
        REQUIRE(p == nullptr || aligned16(p), "mean / sample / tap / v0 not 16-byte aligned");
    const bool draws = (sample != nullptr || tap != nullptr) && (!gauss || add_noise);
    REQUIRE(!draws || rng != nullptr, "sampling needs rng");
    REQUIRE((v0 == nullptr) == (cost_sum == nullptr), "v0 and cost_sum go together");
    REQUIRE(cost_sum == nullptr || aligned16(cost_sum), "cost_sum (4 floats) not 16-byte aligned");
    if (v0) {
        REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
        REQUIRE(workspace_bytes >= partial_floats(B, V) * kF, "workspace of mdbn_absent_visible_workspace_bytes needed");
    }
    AbsentVisibleArgs g{};
    g.pre = pre; g.mean = mean; g.sample = sample; g.tap = tap; g.v0 = v0;
    g.cost_partials = v0 ? reinterpret_cast<float*>(workspace) : nullptr;
    g.observed = observed; g.B = (int)B; g.V = (int)V; g.ld = ldv; g.gauss = gauss != 0; g.add_noise = add_noise != 0;
    mdbn_rng zero{};
    g.rng = make_key(rng ? *rng : zero, rng ? rng->draw : 0u);
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(launch_absent_visible(g, s));
    if (cost_sum)
        HIP_OK(launch_finalize_stats(nullptr, nullptr, nullptr, 0, 0, 0, g.cost_partials, (int)absent_visible_blocks(B, V), nullptr,
                                     nullptr, cost_sum, nullptr, s));
    return MDBN_OK;
}

int mdbn_absent_mark_rows(mdbn_ctx* ctx, void* stream, float* y, int64_t N, int64_t ld, int64_t cols, const int32_t* row_count)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr, "ctx is NULL");
    CHECK(check_shape(N, cols));
    CHECK(check_mat(y, ld, cols, "y"));
    REQUIRE(row_count != nullptr && (reinterpret_cast<uintptr_t>(row_count) & 3u) == 0, "row_count is NULL or not aligned");
    HIP_OK(launch_absent_mark_rows(y, N, ld, cols, row_count, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_cd_step_absent_workspace_bytes(mdbn_ctx* ctx, int64_t B, int64_t V, int64_t H, int64_t ldv, int64_t ldh, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr && bytes != nullptr, "NULL argument");
    CHECK(check_shape(B, V));
    REQUIRE(H > 0, "H must be positive");
    int64_t dense;
    CHECK(step_dense_bytes(B, V, H, ldv, ldh, dense));
    *bytes = dense + (mask_floats(B, V) + partial_floats(B, V)) * kF;
    return MDBN_OK;
}

int mdbn_cd_step_absent(mdbn_ctx* ctx, void* stream, const mdbn_cd_args* a)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr && a != nullptr, "NULL argument");
    REQUIRE(a->struct_size == sizeof(mdbn_cd_args),
            "mdbn_cd_args.struct_size is %llu, this library's struct has %llu bytes (built against another mdbn_hip.h?)",
            (unsigned long long)a->struct_size, (unsigned long long)sizeof(mdbn_cd_args));
    const int64_t B = a->B, V = a->V, H = a->H, ldv = a->ldv, ldh = a->ldh;
    REQUIRE(H > 0 && a->k >= 1, "bad shape / k");
    CHECK(check_shape(B, V));
    REQUIRE(a->persistent == nullptr, "absent visible units: a persistent chain is not supported");
    REQUIRE(!a->sample_stats, "absent visible units: sample_stats is not supported");
    REQUIRE(ldv >= V && ldh >= H && ldv % 4 == 0 && ldh % 4 == 0, "leading dims must be multiples of 4, >= V / H");
    CHECK(check_mat(a->data, ldv, V, "data"));
    CHECK(check_mat(a->W, ldh, H, "W"));
    CHECK(check_mat(a->V2, ldv, V, "V2"));
    CHECK(check_mat(a->P2, ldh, H, "P2"));
    CHECK(check_mat(a->hs, ldh, H, "hs"));
    CHECK(check_mat(a->vs, ldv, V, "vs"));
    REQUIRE(a->hbias && a->vbias, "bias pointers are NULL");
    REQUIRE(a->stats != nullptr && aligned16(a->stats), "stats not aligned");
    REQUIRE(a->indexes != nullptr || B <= a->n_data, "identity minibatch longer than data");
    REQUIRE(a->workspace != nullptr && aligned16(a->workspace), "workspace must be a 16-byte aligned device pointer");
    int64_t dense;
    CHECK(step_dense_bytes(B, V, H, ldv, ldh, dense));
    const int64_t need = dense + (mask_floats(B, V) + partial_floats(B, V)) * kF;
    if (a->workspace_bytes < need)
        return fail(MDBN_ENOSPC, "workspace %lld bytes < the %lld of mdbn_cd_step_absent_workspace_bytes", (long long)a->workspace_bytes,
                    (long long)need);
    Workspace probe;                                   // the statistics' carve-up: refused here, before any launch
    CHECK(carve(a->workspace, dense, B, V, H, probe, true, ldv, ldh));
    Workspace ws;
    CHECK(carve(a->workspace, dense, B, V, H, ws, false));
    uint32_t* observed = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a->workspace) + dense);
    float* partials = reinterpret_cast<float*>(observed) + mask_floats(B, V);
    hipStream_t s = (hipStream_t)stream;
    float *v0 = a->V2, *nv = a->V2 + B * ldv, *ph = a->P2, *nh = a->P2 + B * ldh;
    float* cost = a->stats + V * ldh + ldh + ldv;
    const bool gauss = a->gauss != 0;

    HIP_OK(launch_gather(a->data, a->n_data, ldv, ldv, a->indexes, a->index_is_64, B, v0, ldv, s));
    {                                                                   // O_r, and the rows zero-filled in place
        AbsentSplitArgs sp{};
        sp.x = v0; sp.ldx = ldv; sp.filled = v0; sp.ld_filled = ldv; sp.observed = observed; sp.B = (int)B; sp.V = (int)V;
        HIP_OK(launch_absent_split(sp, s));
    }
    // the kernel leaves pad columns alone; the propup that reads vs wants them zero
    if (ldv > V) HIP_OK(hipMemset2DAsync(a->vs + V, sizeof(float) * ldv, 0, sizeof(float) * (ldv - V), B, s));
    {                                                                   // positive phase: draw 0
        Affine up(v0, B, ldv, a->W, V, H, ldh, a->hbias);
        up.mean = ph; up.sample = a->hs; up.rng = &a->rng;
        CHECK(run_affine(up, ws, s, nullptr));
        if (a->trace_h) HIP_OK(hipMemcpyAsync(a->trace_h, a->hs, sizeof(float) * B * ldh, hipMemcpyDeviceToDevice, s));
    }
    AbsentVisibleArgs g{};
    g.observed = observed; g.B = (int)B; g.V = (int)V; g.ld = ldv; g.gauss = gauss; g.add_noise = a->add_noise != 0;
    for (int t = 1; t <= a->k; ++t) {                                   // gibbs_hvh x k: draws 2t - 1 (visible), 2t (hidden)
        const bool last = t == a->k;
        // the linear pre-activations h W^T + vbias into rows B.. of V2, then the kernel turns them into masked means in place
        Affine down(a->hs, B, ldh, a->W, V, H, ldh, a->vbias, ldv, 1);
        down.mean = nv;
        down.x_binary = true;
        CHECK(run_affine(down, ws, s, nullptr));
        g.pre = nv; g.mean = nv; g.sample = a->vs;
        g.tap = a->trace_v ? a->trace_v + (int64_t)(t - 1) * B * ldv : nullptr;
        g.v0 = last ? v0 : nullptr;
        g.cost_partials = last ? partials : nullptr;
        g.rng = make_key(a->rng, (uint32_t)(2 * t - 1));
        HIP_OK(launch_absent_visible(g, s));
        if (last)
            HIP_OK(launch_finalize_stats(nullptr, nullptr, nullptr, 0, 0, 0, partials, (int)absent_visible_blocks(B, V), nullptr, nullptr,
                                         cost, nullptr, s));
        // h_t | v_t: from the masked mean for a Gaussian layer (the reference's chain), from the masked 0/1 sample otherwise
        Affine up(gauss ? nv : a->vs, B, ldv, a->W, V, H, ldh, a->hbias);
        up.mean = nh; up.sample = last ? nullptr : a->hs; up.mean_scale = -1.0f;
        up.rng = &a->rng; up.draw = (uint32_t)(2 * t);
        up.x_binary = !gauss;
        CHECK(run_affine(up, ws, s, nullptr));
        if (a->trace_h && !last)
            HIP_OK(hipMemcpyAsync(a->trace_h + (int64_t)t * B * ldh, a->hs, sizeof(float) * B * ldh, hipMemcpyDeviceToDevice, s));
    }
    return mdbn_cd_stats(ctx, stream, a->V2, a->P2, B, V, H, ldv, ldh, a->stats, a->workspace, dense);
}

int mdbn_free_energy_absent_workspace_bytes(mdbn_ctx* ctx, int64_t N, int64_t V, int64_t H, int64_t ldv, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr && bytes != nullptr, "NULL argument");
    CHECK(check_shape(N, V));
    REQUIRE(H > 0 && ldv >= V && ldv % 4 == 0, "bad H / ldv");
    int64_t inner;
    CHECK(fe_inner_bytes(N, V, H, inner));
    *bytes = (ru64(N * ldv) + mask_floats(N, V)) * kF + inner;
    return MDBN_OK;
}

int mdbn_free_energy_absent(mdbn_ctx* ctx, void* stream, const float* x, int64_t N, int64_t ldv, const float* W, int64_t V,
                            int64_t H, int64_t ldh, const float* hbias, const float* vbias, int gauss, float* out, void* workspace,
                            int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr, "ctx is NULL");
    CHECK(check_shape(N, V));
    REQUIRE(H > 0, "bad shape");
    CHECK(check_mat(x, ldv, V, "x"));
    CHECK(check_mat(W, ldh, H, "W"));
    REQUIRE(hbias && vbias && out, "NULL pointer");
    REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
    int64_t inner;
    CHECK(fe_inner_bytes(N, V, H, inner));
    const int64_t need = (ru64(N * ldv) + mask_floats(N, V)) * kF + inner;
    if (workspace_bytes < need)
        return fail(MDBN_ENOSPC, "workspace %lld bytes < the %lld of mdbn_free_energy_absent_workspace_bytes", (long long)workspace_bytes,
                    (long long)need);
    float* filled = reinterpret_cast<float*>(workspace);
    uint32_t* observed = reinterpret_cast<uint32_t*>(filled + ru64(N * ldv));
    void* rest = reinterpret_cast<float*>(observed) + mask_floats(N, V);
    hipStream_t s = (hipStream_t)stream;
    // (the kernel leaves the pad columns of the staging rows alone; the propup reads them as zero)
    if (ldv > V) HIP_OK(hipMemset2DAsync(filled + V, sizeof(float) * ldv, 0, sizeof(float) * (ldv - V), N, s));
    AbsentSplitArgs sp{};
    sp.x = x; sp.ldx = ldv; sp.filled = filled; sp.ld_filled = ldv; sp.observed = observed; sp.B = (int)N; sp.V = (int)V;
    HIP_OK(launch_absent_split(sp, s));
    CHECK(mdbn_free_energy(ctx, stream, filled, N, ldv, W, V, H, ldh, hbias, vbias, gauss, out, rest, inner));
    // Gaussian: a zero-filled absent entry added b_i^2 / 2 to the row's energy
    if (gauss) HIP_OK(launch_absent_fe_fix(observed, N, V, vbias, out, s));
    return MDBN_OK;
}

}  // extern "C"

// C-ABI drivers of the learned per-column variance of a Gaussian visible layer (declared in include/mdbn_hip.h): the scaled
// gather and the log-sigma step of mdbn_sigma.hip.  Of the core they use what mdbn_capi_internal.h declares.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "mdbn_capi_internal.h"
#include "mdbn_sigma.h"

using namespace mdbn;
using namespace mdbn::capi;

namespace {

constexpr int64_t kSigmaMaxRows = 1 << 19;          // (slices of the two-stage sum ride on gridDim.y)

int64_t sigma_partial_floats(int64_t B, int64_t V) { return sigma_slices(B) > 1 ? (int64_t)sigma_slices(B) * ru4(V) : 0; }

bool float_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int mdbn_sigma_workspace_bytes(mdbn_ctx* ctx, int64_t B, int64_t V, int64_t* bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && bytes && B > 0 && V > 0 && B <= kSigmaMaxRows && V <= (1 << 24), "bad arguments (0 < B <= 2^19, 0 < V <= 2^24)");
    *bytes = sigma_partial_floats(B, V) * (int64_t)sizeof(float);
    return MDBN_OK;
}

int mdbn_sigma_scale_rows(mdbn_ctx* ctx, void* stream, const float* src, int64_t n_src, int64_t ld_src, const void* indexes,
                          int index_is_64, int64_t B, int64_t V, const float* log_sigma, float sign, float* dst, int64_t ld_dst)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx != nullptr, "ctx is NULL");
    REQUIRE(B > 0 && V > 0 && n_src > 0 && B <= (1 << 24) && V <= (1 << 24), "sizes must be positive (and B, V <= 2^24)");
    CHECK(check_mat(src, ld_src, V, "src"));
    CHECK(check_mat(dst, ld_dst, V, "dst"));
    REQUIRE(log_sigma != nullptr && float_aligned(log_sigma), "log_sigma is NULL or not aligned");
    REQUIRE(indexes != nullptr || B <= n_src, "identity minibatch longer than the source");
    REQUIRE(indexes == nullptr || (reinterpret_cast<uintptr_t>(indexes) & (index_is_64 ? 7u : 3u)) == 0, "indexes not aligned");
    REQUIRE(sign == 1.0f || sign == -1.0f, "sign must be +1 or -1");
    SigmaScaleArgs a{};
    a.src = src; a.n_src = n_src; a.ld_src = ld_src; a.idx = indexes; a.idx64 = index_is_64; a.B = (int)B; a.V = (int)V;
    a.log_sigma = log_sigma; a.sign = sign; a.dst = dst; a.ld_dst = ld_dst;
    HIP_OK(launch_sigma_scale_rows(a, (hipStream_t)stream));
    return MDBN_OK;
}

int mdbn_sigma_update(mdbn_ctx* ctx, void* stream, const float* U, int64_t ldu, const float* M, int64_t ldm, int64_t B, int64_t V,
                      int64_t n_rows, float lr, float momentum, float lo, float hi, float* log_sigma, float* log_sigma_speed,
                      void* workspace, int64_t workspace_bytes)
{
    CtxScope ctx_scope(ctx);
    REQUIRE(ctx && U && M && log_sigma && log_sigma_speed, "null pointer");
    REQUIRE(B > 0 && V > 0 && B <= kSigmaMaxRows && V <= (1 << 24), "sizes must be positive (B <= 2^19, V <= 2^24)");
    REQUIRE(n_rows >= 1 && n_rows <= B, "n_rows = %lld: between 1 and B = %lld", (long long)n_rows, (long long)B);
    CHECK(check_mat(U, ldu, V, "U"));
    CHECK(check_mat(M, ldm, V, "M"));
    REQUIRE(float_aligned(log_sigma) && float_aligned(log_sigma_speed), "log_sigma / log_sigma_speed not aligned");
    REQUIRE(lr >= 0.f && lr <= 3.0e38f, "lr must be finite and not negative");
    REQUIRE(momentum >= 0.f && momentum <= 1.f, "momentum must lie in [0, 1]");
    REQUIRE(lo <= hi && lo >= -3.0e38f && hi <= 3.0e38f, "the clamp needs finite lo <= hi");
    const int64_t need = sigma_partial_floats(B, V) * (int64_t)sizeof(float);
    if (need > 0) {
        REQUIRE(workspace != nullptr && aligned16(workspace), "workspace must be a 16-byte aligned device pointer");
        REQUIRE(workspace_bytes >= need, "workspace of mdbn_sigma_workspace_bytes needed");
    }
    SigmaUpdateArgs a{};
    a.U = U; a.M = M; a.ldu = ldu; a.ldm = ldm; a.n_rows = (int)n_rows; a.V = (int)V; a.n_slices = sigma_slices(n_rows);
    a.lr = lr; a.momentum = momentum; a.lo = lo; a.hi = hi; a.log_sigma = log_sigma; a.speed = log_sigma_speed;
    a.partials = reinterpret_cast<float*>(workspace);
    HIP_OK(launch_sigma_update(a, (hipStream_t)stream));
    return MDBN_OK;
}

}  // extern "C"

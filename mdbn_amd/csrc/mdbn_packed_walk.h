// Device helpers shared by the passes between mdbn_cd_step and mdbn_apply_update (mdbn_center.hip, mdbn_sparsity.hip): the
// column mean of the float32 copies of v0 / ph_mean in the step's scratch, and the walk of a row of the packed statistics
// [S | s_h | s_v | cost] in 16-byte groups that leaves the pad columns alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdbn {

constexpr int COLUMN_MEAN_NT = 64;          // threads of a workgroup that owns one column per thread: one wave

// mean of x[0], x[ld], ..., x[(B - 1) ld]: the rows added in ascending order
__device__ __forceinline__ float column_mean(const float* x, int64_t ld, int B)
{
    // compensated (Kahan) float32 sum: a plain running sum of 512 means in (0, 1) is off by 5e-7 of the mean, and the
    // correction of s_h multiplies an error of lam by mu . s_v, thousands for sparse 0 / 1 data
    float s = 0.f, comp = 0.f;
    auto add = [&](float v) {
        const float y = v - comp, t = s + y;
        comp = (t - s) - y;
        s = t;
    };
    int r = 0;
    for (; r + 32 <= B; r += 32) {           // 32 rows in flight (the walk is latency-bound: one wave per 64 columns), added in ascending order
        float t[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) t[u] = x[(int64_t)(r + u) * ld];
#pragma unroll
        for (int u = 0; u < 32; ++u) add(t[u]);
    }
    for (; r < B; ++r) add(x[(int64_t)r * ld]);
    return s / (float)B;
}

// the floats 0 .. n-1 of a 16-byte group, the others as exact zeros (n = 4: one 16-byte access)
__device__ __forceinline__ float4 load_live(const float* p, int n)
{
    if (n == 4) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    return v;
}

__device__ __forceinline__ float4 load_live_scalar(const float* p, int n)     // a base that need not be 16-byte aligned
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    if (n > 3) v.w = p[3];
    return v;
}

__device__ __forceinline__ void store_live(float* p, int n, float4 v)
{
    if (n == 4) { *reinterpret_cast<float4*>(p) = v; return; }
    if (n > 0) p[0] = v.x;
    if (n > 1) p[1] = v.y;
    if (n > 2) p[2] = v.z;
}

}  // namespace mdbn

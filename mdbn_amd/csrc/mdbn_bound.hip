// Device pieces of the variational lower bound on log p(data) of a DBN (Salakhutdinov & Murray 2008, section 4.2;
// DBN.log_likelihood_bound):
//
//   rowll_kernel            the directed term log p(x_{l-1} | x_l) of every replica row: the propdown GEMM h W^T on the bf16
//                           matrix pipe whose output tile never leaves the accumulators -- the epilogue adds the visible bias,
//                           forms t pre - softplus(pre) (or (t - pre)^2) against the target row and sums it over the tile's
//                           columns; rowll_finish_kernel adds the column tiles of a row in a fixed order.  No atomics: two
//                           runs agree bit for bit.
//   sample_replicas_kernel  S Bernoulli samples of every row of a mean matrix, addressed like mdbn_rng_uniform on the
//                           [N S, H] replica matrix, and the entropy of the factorial distribution of every row.
//
// The GEMM is NT (both operands contiguous along H).  h holds 0 / 1 and is exactly one bf16 piece; W is split into its
// three exact bf16 pieces on the way into LDS (mdbn_bf16x3.h): three v_mfma_f32_32x32x16_bf16 products per fragment pair with
// f32 accumulation, the arithmetic of the plane propdown for 0 / 1 operands.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_bound.h"
#include "mdbn_bf16x3.h"
#include "mdbn_device.h"

namespace mdbn {
namespace {

constexpr int LDK = ROWLL_BK + 8;            // bf16 per staged row: 80 bytes, so that the 16-byte fragment reads of 16 rows fall on 16 different slots
constexpr int PLANE = ROWLL_BM * LDK;        // elements of one staged piece (ROWLL_BM == ROWLL_BN rows)
constexpr int LDT = 65;                      // floats per row of the term tile (64 + 1: a thread per row walks it without conflicts)
static_assert(ROWLL_BM == ROWLL_BN && ROWLL_BM == 128 && ROWLL_BK == 32 && ROWLL_NT == 256, "the loader and wave maps below are written for this shape");
static_assert(ROWLL_BM * LDT * (int)sizeof(float) <= 4 * PLANE * (int)sizeof(unsigned short), "the term tile reuses the staging area");

// four floats k .. k + 3 of a row whose storage is ld floats long (ld % 4 == 0, k % 4 == 0), entries at k >= H as exact zeros:
// whatever the padding holds (NaN included) never reaches a product
__device__ __forceinline__ float4 rowll_load4(const float* row, int k, int H, int64_t ld)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < ld) v = *reinterpret_cast<const float4*>(row + k);
    v.x = k < H ? v.x : 0.f;
    v.y = k + 1 < H ? v.y : 0.f;
    v.z = k + 2 < H ? v.z : 0.f;
    v.w = k + 3 < H ? v.w : 0.f;
    return v;
}

__device__ __forceinline__ unsigned hi16_pair(float lo, float hi)      // (hi16(hi) << 16) | hi16(lo)
{
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, hi), __builtin_bit_cast(unsigned, lo), 0x07060302u);
}

template <bool GAUSS>
__global__ __launch_bounds__(ROWLL_NT) void rowll_kernel(RowllArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned short stage[4 * PLANE];      // [h | W piece 1 | 2 | 3][128][LDK]; then the term tile
    __shared__ int trow[ROWLL_BM];                                                // target row of every tile row
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int tn = (int)blockIdx.x % a.tiles_n, tm = (int)blockIdx.x / a.tiles_n;
    const int m0 = tm * ROWLL_BM, n0 = tn * ROWLL_BN;
    if (tid < ROWLL_BM) trow[tid] = min(m0 + tid, a.R - 1) / a.target_div;

    // loader: thread = (row lr + 32 u, floats 4 c4 .. 4 c4 + 3) of both operands' stage; rows past the end read the last row
    // (their results are never stored)
    const int c4 = tid & 7, lr = tid >> 3;
    const float* arow[4];
    const float* brow[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        arow[u] = a.h + (int64_t)min(m0 + lr + 32 * u, a.R - 1) * a.ldh;
        brow[u] = a.W + (int64_t)min(n0 + lr + 32 * u, a.V - 1) * a.ldh;
    }
    float4 xa[4], xb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + 4 * c4;
#pragma unroll
        for (int u = 0; u < 4; ++u) xa[u] = rowll_load4(arow[u], k, a.H, a.ldh);
#pragma unroll
        for (int u = 0; u < 4; ++u) xb[u] = rowll_load4(brow[u], k, a.H, a.ldh);
    };
    auto park = [&]() {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int off = (lr + 32 * u) * LDK + 4 * c4;
            *reinterpret_cast<uint2*>(stage + off) = make_uint2(hi16_pair(xa[u].x, xa[u].y), hi16_pair(xa[u].z, xa[u].w));
            unsigned p1, p2, p3, q1, q2, q3;
            th_split2(xb[u].x, xb[u].y, p1, p2, p3);
            th_split2(xb[u].z, xb[u].w, q1, q2, q3);
            *reinterpret_cast<uint2*>(stage + PLANE + off) = make_uint2(p1, q1);
            *reinterpret_cast<uint2*>(stage + 2 * PLANE + off) = make_uint2(p2, q2);
            *reinterpret_cast<uint2*>(stage + 3 * PLANE + off) = make_uint2(p3, q3);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[x][y][e] = 0.f;

    fetch(0);
    for (int k0 = 0; k0 < a.H; k0 += ROWLL_BK) {
        __syncthreads();                     // the previous stage's fragments have been read
        park();
        __syncthreads();
        if (k0 + ROWLL_BK < a.H) fetch(k0 + ROWLL_BK);      // in flight under this stage's MFMAs
#pragma unroll
        for (int ks = 0; ks < ROWLL_BK / 16; ++ks) {
            const int kof = 16 * ks + 8 * hh;
            tbf16x8 fa[2], fb[2][3];
#pragma unroll
            for (int x = 0; x < 2; ++x) fa[x] = *reinterpret_cast<const tbf16x8*>(stage + (64 * wm + 32 * x + i) * LDK + kof);
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    fb[y][pl] = *reinterpret_cast<const tbf16x8*>(stage + (1 + pl) * PLANE + (64 * wn + 32 * y + i) * LDK + kof);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {          // smallest piece first, as th_mma<1>
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[x], fb[y][2], acc[x][y], 0, 0, 0);
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[x], fb[y][1], acc[x][y], 0, 0, 0);
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[x], fb[y][0], acc[x][y], 0, 0, 0);
                }
        }
    }

    // epilogue on the accumulators: lane (i, hh) of wave (wm, wn) holds column n0 + 64 wn + 32 y + i of the rows
    // 64 wm + 32 x + (e & 3) + 8 (e >> 2) + 4 hh.  Columns >= V count as 0 (they were computed from the last live row of W).
    __syncthreads();                         // every wave is done with the staged pieces: the area becomes the term tile
    float* T = reinterpret_cast<float*>(stage);
    int col[2];
    bool live[2];
    float vb[2];
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        const int c = n0 + 64 * wn + 32 * y + i;
        live[y] = c < a.V;
        col[y] = min(c, a.V - 1);
        vb[y] = a.vbias[col[y]];
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rl = 64 * wm + 32 * x + (e & 3) + 8 * (e >> 2) + 4 * hh;
            const float* trg = a.target + (int64_t)trow[rl] * a.ldv;
            float s = 0.f;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const float t = trg[col[y]];
                const float pre = acc[x][y][e] + vb[y];
                float term;
                if constexpr (GAUSS) { const float d = t - pre; term = d * d; }
                else term = t * pre - softplusf_(pre);
                s += live[y] ? term : 0.f;
            }
            T[rl * LDT + 32 * wn + i] = s;
        }
    }
    __syncthreads();
    if (tid < ROWLL_BM && m0 + tid < a.R) {  // a row's 64 lane sums in ascending column order
        float s = 0.f;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) s += T[tid * LDT + j];
        a.partial[(int64_t)tn * a.R + m0 + tid] = s;
    }
}

// out[r] = the column tiles of row r added in ascending order (and the Gaussian constants)
__global__ __launch_bounds__(256) void rowll_finish_kernel(RowllArgs a)
{
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r >= a.R) return;
    float s = 0.f;
    for (int t = 0; t < a.tiles_n; ++t) s += a.partial[(int64_t)t * a.R + r];
    a.out[r] = a.gauss ? -0.5f * s - 0.91893853320467274178f * (float)a.V : s;
}

// thread = (Philox block q = global rows 4 q .. 4 q + 3, column j): one block serves four replica rows, which may belong to
// different data rows
__global__ __launch_bounds__(256) void sample_replicas_kernel(ReplicaArgs a, int64_t q0, int64_t nq)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nq * a.ldh) return;
    const int64_t q = q0 + idx / a.ldh, j = idx % a.ldh;
    const bool live = j < a.H;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (live) philox4x32_10((uint32_t)j, (uint32_t)q, a.rng.draw, a.rng.step, a.rng.k0, a.rng.k1, w);
    const int64_t rows = a.N * a.S;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t loc = 4 * q + r - (int64_t)a.rng.row_offset;
        if (loc < 0 || loc >= rows) continue;
        float sv = 0.f;
        if (live) sv = philox_u01(w[r]) < a.mean[(loc / a.S) * a.ldh + j] ? 1.0f : 0.0f;
        a.sample[loc * a.ldh + j] = sv;
    }
}

// one wave per data row; lane sums over columns lane, lane + 64, ... combined by a fixed butterfly
__global__ __launch_bounds__(256) void replica_entropy_kernel(ReplicaArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= a.N) return;
    const float* m = a.mean + n * a.ldh;
    float s = 0.f;
    for (int64_t j = lane; j < a.H; j += 64) {
        const float p = m[j];
        float t = 0.f;
        if (p > 0.f) t += p * logf(p);
        if (p < 1.f) t += (1.0f - p) * logf(1.0f - p);
        s += t;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) a.entropy[n] = -s;
}

}  // namespace

hipError_t launch_rowll(const RowllArgs& a, hipStream_t s)
{
    if (a.R < 1 || a.V < 1 || a.H < 1 || a.target_div < 1 || a.tiles_m != (a.R + ROWLL_BM - 1) / ROWLL_BM ||
        a.tiles_n != (a.V + ROWLL_BN - 1) / ROWLL_BN || (int64_t)a.tiles_m * a.tiles_n > 0x7fffffff || a.ldh < a.H || a.ldv < a.V ||
        (a.ldh & 3))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.tiles_m * a.tiles_n));
    if (a.gauss) hipLaunchKernelGGL(rowll_kernel<true>, grid, dim3(ROWLL_NT), 0, s, a);
    else hipLaunchKernelGGL(rowll_kernel<false>, grid, dim3(ROWLL_NT), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rowll_finish_kernel, dim3((unsigned)((a.R + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sample_replicas(const ReplicaArgs& a, hipStream_t s)
{
    if (a.N < 1 || a.S < 1 || a.H < 1 || a.ldh < a.H) return hipErrorInvalidValue;
    const int64_t first = (int64_t)a.rng.row_offset, last = first + a.N * a.S - 1;
    const int64_t q0 = first >> 2, nq = (last >> 2) - q0 + 1;
    const int64_t blocks = (nq * a.ldh + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_replicas_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, q0, nq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.entropy) return e;
    hipLaunchKernelGGL(replica_entropy_kernel, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdbn

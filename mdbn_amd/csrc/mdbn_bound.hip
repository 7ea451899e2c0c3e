// Device pieces of the variational lower bound on log p(data) of a DBN (Salakhutdinov & Murray 2008, section 4.2;
// DBN.log_likelihood_bound):
//
//   rowll_kernel            the directed term log p(x_{l-1} | x_l) of every replica row: the propdown GEMM h W^T on the bf16
//                           matrix pipe whose output tile never leaves the accumulators -- the epilogue adds the visible bias,
//                           forms t pre - softplus(pre) (or (t - pre)^2) against the target row and sums it over the tile's
//                           columns; rowll_finish_kernel adds the column tiles of a row in a fixed order.  No atomics: two
//                           runs agree bit for bit.
//   rowll_grouped_kernel    the same term for a layer whose visible columns hold softmax groups: the same main loop, an
//                           epilogue that forms a group's log-sum-exp from the tile's pre-activations in LDS, and
//                           rowll_grouped_finish_kernel, which also joins the two parts of a group cut by a tile's edge.
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

// ------------------------------------------------------------------ softmax groups in the visible layer
constexpr int GHALF = ROWLL_BM / 2;          // rows of one group pass: the tile's pre-activations go through LDS in two halves
constexpr int LDP = ROWLL_BN + 1;            // floats per row of the pre-activation half tile
constexpr int GUNITS = ROWLL_BN / 2 + 1;     // groups that touch one tile: a head fragment and 64 groups of two columns
constexpr int GCHUNK = 32;                   // columns of a row that one thread of the group pass holds: four threads per row
static_assert(GHALF * LDP * (int)sizeof(float) <= 4 * PLANE * (int)sizeof(unsigned short), "the half tile reuses the staging area");
static_assert(4 * GCHUNK == ROWLL_BN && 4 * GHALF == ROWLL_NT, "the group pass: 64 rows x 4 chunks of 32 columns = 256 threads");

// (max, sum of exp(x - max)) of the union of two sets of pre-activations; a sum of 0 is the empty set
__device__ __forceinline__ void lse_join(float& m, float& z, float m2, float z2)
{
    if (z2 <= 0.f) return;
    if (z <= 0.f) { m = m2; z = z2; return; }
    const float M = fmaxf(m, m2);
    z = z * __expf(m - M) + z2 * __expf(m2 - M);
    m = M;
}

// entry j of the device table, held to the span the host copy gives
__device__ __forceinline__ int group_boundary(const RowllGroupArgs& g, int j)
{
    return min(max(g.group_start[j], g.span_lo), g.span_hi);
}

// The first j in [0, n_groups + 1) whose boundary is > x (n_groups + 1: none), by one wave: every round 64 lanes probe the
// ends of 64 equal pieces of the range and a ballot picks the piece -- two dependent loads for a table of 4096 entries.
// Wave-uniform; ends for any table contents.
__device__ __forceinline__ int first_boundary_above(const RowllGroupArgs& g, int x, int lane)
{
    int lo = 0, hi = g.n_groups + 1;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int p = lo + lane * step + step - 1;
        const bool above = p >= hi || group_boundary(g, p) > x;
        const unsigned long long b = __ballot(above);
        if (b == 0ull) { lo = hi; break; }
        const int first = lo + (__ffsll(b) - 1) * step;
        hi = min(first + step - 1, hi);
        lo = first;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// rowll_kernel's main loop, copied statement for statement (that kernel keeps its own, so that its code generation stays
// what it was measured with): acc = the 64 x 64 block of h W^T of this wave (2 x 2 fragments of 32 x 32) over all K stages.
// stage: [h | W piece 1 | 2 | 3][128][LDK]; on return some waves may still be reading it.  (tid, i, hh, wm, wn: the
// thread's place as the kernel computes it)
__device__ __forceinline__ void rowll_grouped_mainloop(const RowllArgs& a, unsigned short* stage, int m0, int n0, int tid, int i, int hh, int wm,
                                               int wn, f32x16 (&acc)[2][2])
{
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
}

// rowll_kernel<false> with a grouped epilogue, in two parts.
// (1) rowll_kernel's own epilogue on the accumulators, by all four waves at once, for what is linear in or local to a
//     column: t pre of every column and -softplus(pre) of the columns outside the span, summed per row.
// (2) The log-sum-exp of a group needs the columns of a row side by side.  Per half of the tile's rows the two waves that
//     hold it store pre (bias added) to LDS; then thread (row, q) of all 256 loads the 32 columns 32 q .. 32 q + 31 of its
//     row into registers and walks them once: a running (max, sum of exp(pre - max)) per group, one exponential per column,
//     started and closed by three bit masks of the tile (bit c of word q: column 32 q + c begins a group / ends one / lies
//     in one), which wave 0 makes from the table before the main loop.  What a thread cannot close -- a group that began
//     left of its 32 columns or goes on to their right -- it hands over as (max, sum); the four threads of a row join these
//     in column order, and what is still open at the tile's edge goes to rowll_grouped_finish_kernel.
// A tile without a group column skips (2).
__global__ __launch_bounds__(ROWLL_NT) void rowll_grouped_kernel(RowllGroupArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned short stage[4 * PLANE];      // the staged pieces; then the term tile; then [64][LDP] pre
    __shared__ int trow[ROWLL_BM];
    __shared__ float rowsum[ROWLL_BM];                                            // part (1) of every tile row
    __shared__ unsigned gmask[3][4];                                              // begins / ends / lies in a group: bit c of word q = column 32 q + c
    __shared__ int meta[2];                                                       // groups that touch the tile; the first one began in the previous tile
    const RowllArgs& a = g.a;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int tn = (int)blockIdx.x % a.tiles_n, tm = (int)blockIdx.x / a.tiles_n;
    const int m0 = tm * ROWLL_BM, n0 = tn * ROWLL_BN;
    if (tid < ROWLL_BM) trow[tid] = min(m0 + tid, a.R - 1) / a.target_div;

    // the groups of this tile, g0 .. g0 + nu - 1: from the first that ends behind n0 to the last that begins before the
    // tile's end.  Every column taken from the table is held to [0, columns of the tile]; the masks are read by every thread
    // after the main loop's barriers.
    if (wave == 0) {
        const int nend = min(n0 + ROWLL_BN, a.V), ncol = nend - n0;
        const int g0 = max(first_boundary_above(g, n0, lane) - 1, 0);
        const int g1 = min(first_boundary_above(g, nend - 1, lane), g.n_groups);
        const int nu = min(max(g1 - g0, 0), GUNITS);
        if (lane < 12) (&gmask[0][0])[lane] = 0u;
        __builtin_amdgcn_wave_barrier();     // (one wave: its LDS operations take effect in program order)
        for (int j = lane; j < nu; j += 64) {
            const int b0 = group_boundary(g, g0 + j), b1 = group_boundary(g, g0 + j + 1);
            const int cs = min(max(b0 - n0, 0), ncol), ce = min(max(b1 - n0, 0), ncol);
            if (ce <= cs) continue;
            if (b0 >= n0) atomicOr(&gmask[0][cs >> 5], 1u << (cs & 31));          // (a group that began before the tile has no beginning here)
            if (b1 <= nend) atomicOr(&gmask[1][(ce - 1) >> 5], 1u << ((ce - 1) & 31));
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int lo = max(cs, 32 * w), hi = min(ce, 32 * w + 32);
                if (lo < hi) atomicOr(&gmask[2][w], (hi - lo == 32 ? ~0u : (1u << (hi - lo)) - 1u) << (lo - 32 * w));
            }
        }
        if (lane == 0) {
            meta[0] = nu;
            meta[1] = nu > 0 && group_boundary(g, g0) < n0;
        }
    }

    f32x16 acc[2][2];
    rowll_grouped_mainloop(a, stage, m0, n0, tid, i, hh, wm, wn, acc);

    // (1) lane (i, hh) of wave (wm, wn) holds column n0 + 64 wn + 32 y + i of the rows 64 wm + 32 x + (e & 3) + 8 (e >> 2) + 4 hh.
    // Columns >= V count as 0 (they were computed from the last live row of W).
    __syncthreads();                         // every wave is done with the staged pieces: the area becomes the term tile
    float* T = reinterpret_cast<float*>(stage);
    int col[2];
    bool live[2], grouped[2];
    float vb[2];
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        const int c = n0 + 64 * wn + 32 * y + i;
        live[y] = c < a.V;
        grouped[y] = c >= g.span_lo && c < g.span_hi;
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
                const float term = grouped[y] ? t * pre : t * pre - softplusf_(pre);
                s += live[y] ? term : 0.f;
            }
            T[rl * LDT + 32 * wn + i] = s;
        }
    }
    __syncthreads();
    const int nu = meta[0];
    const bool head = meta[1] != 0;
    const int64_t R = a.R;
    float* const part = a.partial + (int64_t)tn * ROWLL_GP * R;
    if (tid < ROWLL_BM) {                    // a row's 64 lane sums in ascending column order
        float s = 0.f;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) s += T[tid * LDT + j];
        rowsum[tid] = s;
        if (nu == 0 && m0 + tid < a.R) {
            float* o = part + m0 + tid;
            o[0] = s; o[R] = 0.f; o[2 * R] = 0.f; o[3 * R] = 0.f; o[4 * R] = 0.f;
        }
    }
    if (nu == 0) return;                     // (the whole workgroup)

    // (2)
    float* P = reinterpret_cast<float*>(stage);
    const int rl = tid >> 2, q = tid & 3;
    const unsigned begins = gmask[0][q], ends = gmask[1][q], inside = gmask[2][q];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        __syncthreads();                     // the term tile / the first half has been read
        if (wm == half) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int e = 0; e < 16; ++e)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        P[(32 * x + (e & 3) + 8 * (e >> 2) + 4 * hh) * LDP + 64 * wn + 32 * y + i] = acc[x][y][e] + vb[y];
        }
        __syncthreads();
        float xs[GCHUNK];
#pragma unroll
        for (int c = 0; c < GCHUNK; ++c) xs[c] = P[rl * LDP + GCHUNK * q + c];
        // m, z: the group that is open at column c; own: it began in this thread's columns.  lse: the groups that began
        // and ended here; (hm, hz): the group that ended here and began further left.
        float m = -INFINITY, z = 0.f, lse = 0.f, hm = 0.f, hz = 0.f;
        bool own = false;
#pragma unroll
        for (int c = 0; c < GCHUNK; ++c) {
            const bool in = (inside >> c) & 1u;
            if ((begins >> c) & 1u) { m = -INFINITY; z = 0.f; own = true; }
            // the running pair takes x: exp(-|x - m|) is the one factor that is not 1 (m = -inf: it is 0 and z becomes 1)
            const float d = xs[c] - m, f = __expf(-fabsf(d));
            const float zn = d > 0.f ? fmaf(z, f, 1.0f) : z + f;
            z = in ? zn : z;
            m = in ? fmaxf(m, xs[c]) : m;
            if ((ends >> c) & 1u) {
                if (own) lse += m + __logf(z);
                else { hm = m; hz = z; }
                m = -INFINITY; z = 0.f; own = true;
            }
        }
        const bool through = z > 0.f && !own;            // one group from before the first column to behind the last
        // the four threads of a row, in column order (every one of them computes the same)
        float total = 0.f, cm = 0.f, cz = 0.f, Hm = 0.f, Hz = 0.f;
        bool first = head;                   // the group that began in the previous tile has not ended yet
        const int base = lane & ~3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lse_j = __shfl(lse, base + j, 64), hm_j = __shfl(hm, base + j, 64), hz_j = __shfl(hz, base + j, 64);
            const float m_j = __shfl(m, base + j, 64), z_j = __shfl(z, base + j, 64);
            const bool through_j = __shfl((int)through, base + j, 64) != 0;
            if (hz_j > 0.f) {                // a group ends here that began further left: with what was carried over
                lse_join(cm, cz, hm_j, hz_j);
                if (first) { Hm = cm; Hz = cz; }
                else total += cm + __logf(cz);
                first = false;
                cm = 0.f; cz = 0.f;
            }
            total += lse_j;
            if (through_j) lse_join(cm, cz, m_j, z_j);
            else { cm = z_j > 0.f ? m_j : 0.f; cz = z_j; }
        }
        const int r = m0 + GHALF * half + rl;
        if (q == 0 && r < a.R) {
            float* o = part + r;
            o[0] = rowsum[GHALF * half + rl] - total;
            o[R] = Hm; o[2 * R] = Hz;       // the head fragment, and what is still open behind the last column: the tail
            o[3 * R] = cm; o[4 * R] = cz;
        }
    }
}

// out[r] = the tile sums of row r in ascending order; the tail fragment of a tile and the head fragment of the next are the
// two parts of one group: -(M + log(s_a e^(m_a - M) + s_b e^(m_b - M))), M = max(m_a, m_b)
__global__ __launch_bounds__(256) void rowll_grouped_finish_kernel(RowllArgs a)
{
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r >= a.R) return;
    const int64_t R = a.R;
    float s = 0.f, cm = 0.f, cs = 0.f;       // the fragment carried over from the previous tile (cs == 0: none)
    for (int t = 0; t < a.tiles_n; ++t) {
        const float* p = a.partial + (int64_t)t * ROWLL_GP * R + r;
        s += p[0];
        const float hm = p[R], hs = p[2 * R];
        if (hs > 0.f || cs > 0.f) {
            const float M = cs > 0.f ? (hs > 0.f ? fmaxf(cm, hm) : cm) : hm;
            float z = 0.f;
            if (cs > 0.f) z += cs * expf(cm - M);
            if (hs > 0.f) z += hs * expf(hm - M);
            s -= M + logf(z);
        }
        cm = p[3 * R];
        cs = p[4 * R];
    }
    if (cs > 0.f) s -= cm + logf(cs);
    a.out[r] = s;
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

hipError_t launch_rowll_grouped(const RowllGroupArgs& g, hipStream_t s)
{
    const RowllArgs& a = g.a;
    if (a.R < 1 || a.V < 1 || a.H < 1 || a.target_div < 1 || a.gauss || a.tiles_m != (a.R + ROWLL_BM - 1) / ROWLL_BM ||
        a.tiles_n != (a.V + ROWLL_BN - 1) / ROWLL_BN || (int64_t)a.tiles_m * a.tiles_n > 0x7fffffff || a.ldh < a.H || a.ldv < a.V ||
        (a.ldh & 3) || !g.group_start || g.n_groups < 1 || g.span_lo < 0 || g.span_hi > a.V || g.span_lo > g.span_hi)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rowll_grouped_kernel, dim3((unsigned)(a.tiles_m * a.tiles_n)), dim3(ROWLL_NT), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rowll_grouped_finish_kernel, dim3((unsigned)((a.R + 255) / 256)), dim3(256), 0, s, a);
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

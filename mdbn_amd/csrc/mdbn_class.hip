// Classification RBM kernels (mdbn_class.h says what they compute):
//   class_prep_kernel      x~ (the rows with the label block set to zero) and the stacked visible operand of the statistics GEMM
//   class_forward_kernel   posterior, log p(y* | x), the operand rows w r_pos / -w r_bar and the per-workgroup partials of T, n, nll
//   class_patch_kernel     the partials summed in ascending workgroup order and applied to the packed statistics
// The work of class_forward is B K H evaluations of exp and log / rcp and no matrix product: two passes over (y, j) per row --
// the scores, then the softmax over K, then the weighted sigmoids recomputed --, nothing of size [B, K, H] is ever stored.  Every
// element takes e = exp(-|z|) once: softplus(z) = max(z, 0) + log1p(e), sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e), finite
// for any finite z.  No atomics, every sum in a fixed order: two runs agree bit for bit.  Pad columns H..ldh-1 of A, U and
// V..ldv-1 of the rows are never read.
#include "mdbn_class.h"

namespace mdbn {
namespace {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// The scores: a class's score is a sum of H softplus terms, some hundreds in size, and the posterior lives on the DIFFERENCES of
// the K scores -- a float32 sum would round them at 1e-5.  So the terms are float32 at full precision (expf / log1pf, not the
// hardware approximations) and their sum is carried in float64 from the first add to the softmax.
__device__ __forceinline__ float softplus_z(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoid_e(float z, float e)
{
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    return z >= 0.0f ? r : e * r;
}

__global__ __launch_bounds__(256) void class_prep_kernel(ClassPrepArgs a)
{
    const int64_t j = 4 * ((int64_t)blockIdx.y * 256 + threadIdx.x);
    if (j >= a.ldv) return;
    const int chunk = blockIdx.x;
    const int r0 = chunk * CLASS_PREP_ROWS, r1 = min(r0 + CLASS_PREP_ROWS, a.B);
    const int lv = (int)min((int64_t)4, max((int64_t)0, (int64_t)a.V - j));      // live columns of this quad
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; ++r) {
        const int64_t off = (int64_t)r * a.ldv + j;
        float x[4] = {0.f, 0.f, 0.f, 0.f}, n[4] = {0.f, 0.f, 0.f, 0.f};
        if (lv == 4) {
            const float4 q = *reinterpret_cast<const float4*>(a.v0 + off);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            if (a.nv) {
                const float4 m = *reinterpret_cast<const float4*>(a.nv + off);
                n[0] = m.x; n[1] = m.y; n[2] = m.z; n[3] = m.w;
            }
        } else {
            for (int c = 0; c < lv; ++c) {
                x[c] = a.v0[off + c];
                if (a.nv) n[c] = a.nv[off + c];
            }
        }
        float t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t col = j + c;
            t[c] = (col >= a.lo && col < (int64_t)a.lo + a.K) ? 0.0f : x[c];
            sum[c] += x[c] - n[c];
        }
        const float4 xq = make_float4(x[0], x[1], x[2], x[3]);
        if (a.copy0) *reinterpret_cast<float4*>(a.copy0 + off) = xq;
        if (a.copy1) *reinterpret_cast<float4*>(a.copy1 + off) = xq;
        if (a.copy_nv) *reinterpret_cast<float4*>(a.copy_nv + off) = make_float4(n[0], n[1], n[2], n[3]);
        *reinterpret_cast<float4*>(a.xt + off) = make_float4(t[0], t[1], t[2], t[3]);
    }
    if (a.svp) *reinterpret_cast<float4*>(a.svp + (int64_t)chunk * a.ldv + j) = make_float4(sum[0], sum[1], sum[2], sum[3]);
}

__global__ __launch_bounds__(CLASS_NT) void class_forward_kernel(ClassForwardArgs a)
{
    __shared__ double red[CLASS_NW][CLASS_R][MDBN_GROUP_MAX];
    __shared__ float p[CLASS_R][MDBN_GROUP_MAX];
    __shared__ float logp_s[CLASS_R];
    __shared__ int ystar[CLASS_R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, K = a.K, H = a.H, R = a.R;
    const int64_t ldh = a.ldh;
    const int n_batches = (a.B + R - 1) / R;
    const bool train = a.rpos != nullptr;
    float n_acc = 0.f, nll_acc = 0.f;
    bool first = true;

    for (int b = g; b < n_batches; b += a.G) {
        const int r0 = b * R, nr = min(R, a.B - r0);
        const float* A0 = a.A + (int64_t)r0 * ldh;
        // first pass: a[y] - d[y] = sum_j softplus(A[j] + U[y][j]), one class after the other
        for (int y = 0; y < K; ++y) {
            const float* Uy = a.U + (int64_t)y * ldh;
            double acc[CLASS_R];
#pragma unroll
            for (int r = 0; r < CLASS_R; ++r) acc[r] = 0.0;
            for (int j = tid; j < H; j += CLASS_NT) {
                const float u = Uy[j];
#pragma unroll
                for (int r = 0; r < CLASS_R; ++r)
                    if (r < nr) {
                        acc[r] += (double)softplus_z(A0[(int64_t)r * ldh + j] + u);
                    }
            }
#pragma unroll
            for (int r = 0; r < CLASS_R; ++r) {
                const double t = wave_sum(acc[r]);
                if (lane == 0) red[wave][r][y] = t;
            }
        }
        __syncthreads();
        // the softmax over the K classes of row r0 + wave: lane y holds class y; the waves' sums in ascending order
        if (wave < nr) {
            const int r = wave;
            double sc = -INFINITY;
            if (lane < K) {
                double t = red[0][r][lane];
#pragma unroll
                for (int w = 1; w < CLASS_NW; ++w) t += red[w][r][lane];
                sc = (double)a.d[lane] + t;
            }
            const double m = wave_max(sc);
            const float rel = (float)(sc - m);                             // <= 0: the class's score below the row's largest
            const float e = lane < K ? expf(rel) : 0.f;
            const float Z = wave_sum(e);
            const float pv = e / Z;
            const bool hot = a.label != nullptr && lane < K && a.label[(int64_t)(r0 + r) * a.ld_label + lane] > 0.5f;
            const unsigned long long bal = __ballot(hot);
            const int ys = bal ? (int)__ffsll((long long)bal) - 1 : -1;
            const float lp = __shfl(rel, max(ys, 0), 64) - logf(Z);
            if (lane < K) {
                p[r][lane] = pv;
                if (a.post) a.post[(int64_t)(r0 + r) * a.ldk + lane] = pv;
            }
            if (lane == 0) {
                ystar[r] = ys;
                logp_s[r] = ys >= 0 ? lp : 0.f;
                if (a.logp && ys >= 0) a.logp[r0 + r] = lp;
            }
        }
        __syncthreads();
        if (train) {
            if (tid < K)
                for (int r = 0; r < nr; ++r) n_acc += (tid == ystar[r] ? 1.0f : 0.0f) - p[r][tid];
            if (tid == 0)
                for (int r = 0; r < nr; ++r) nll_acc -= logp_s[r];
            // second pass: the sigmoids again, weighted; a thread keeps its column of the batch's rows in registers and
            // finishes one class's slice of T before the next
            for (int j = tid; j < (int)ldh; j += CLASS_NT) {
                if (j >= H) {                                               // our own operand rows: pad columns zero
                    for (int r = 0; r < nr; ++r) {
                        const int64_t off = (int64_t)(r0 + r) * ldh + j;
                        a.rpos[off] = 0.f; a.rbar[off] = 0.f;
                        if (a.ph) { a.ph_out[off] = 0.f; a.nh_out[off] = 0.f; }
                    }
                    continue;
                }
                float Ar[CLASS_R], rb[CLASS_R], rp[CLASS_R];
#pragma unroll
                for (int r = 0; r < CLASS_R; ++r) {
                    Ar[r] = r < nr ? A0[(int64_t)r * ldh + j] : 0.f;
                    rb[r] = 0.f; rp[r] = 0.f;
                }
                for (int y = 0; y < K; ++y) {
                    const float u = a.U[(int64_t)y * ldh + j];
                    float tacc = 0.f;
#pragma unroll
                    for (int r = 0; r < CLASS_R; ++r)
                        if (r < nr) {
                            const float z = Ar[r] + u;
                            const float s = sigmoid_e(z, __expf(-fabsf(z)));
                            const float ps = p[r][y] * s;
                            rb[r] += ps; tacc += ps;
                            if (y == ystar[r]) rp[r] = s;
                        }
                    float* tp = a.Tp + ((int64_t)g * K + y) * ldh + j;
                    *tp = first ? tacc : *tp + tacc;
                }
#pragma unroll
                for (int r = 0; r < CLASS_R; ++r)
                    if (r < nr) {
                        const int64_t off = (int64_t)(r0 + r) * ldh + j;
                        a.rpos[off] = a.w * rp[r];
                        a.rbar[off] = -a.w * rb[r];
                        if (a.ph) { a.ph_out[off] = a.gen * a.ph[off]; a.nh_out[off] = a.gen * a.nh[off]; }
                    }
            }
            first = false;
        }
        __syncthreads();                                                    // red / p / ystar are rewritten by the next batch
    }
    if (train) {
        if (tid < K) a.np[(int64_t)g * MDBN_GROUP_MAX + tid] = n_acc;
        if (tid == 0) a.nllp[g] = nll_acc;
    }
}

__global__ __launch_bounds__(256) void class_patch_kernel(ClassPatchArgs a, int h_blocks, int t_blocks)
{
    const int blk = blockIdx.x, tid = threadIdx.x;
    if (blk < t_blocks) {                                                   // S[lo + y][j] -= w T[y][j]
        const int y = blk / h_blocks, j = (blk - y * h_blocks) * 256 + tid;
        if (j < a.H) {
            float t = 0.f;
            for (int g = 0; g < a.G; ++g) t += a.Tp[((int64_t)g * a.K + y) * a.ldh + j];
            float* s = a.S + (int64_t)(a.lo + y) * a.ldh + j;
            *s -= a.w * t;
        }
        return;
    }
    const int i = (blk - t_blocks) * 256 + tid;                             // s_v rebuilt whole
    if (i < a.V) {
        float acc = 0.f;
        if (a.svp)
            for (int c = 0; c < a.chunks; ++c) acc += a.svp[(int64_t)c * a.ldv + i];
        float v = a.gen * acc;
        if (i >= a.lo && i < a.lo + a.K) {
            float n = 0.f;
            for (int g = 0; g < a.G; ++g) n += a.np[(int64_t)g * MDBN_GROUP_MAX + (i - a.lo)];
            v += a.w * n;
        }
        a.s_v[i] = v;
    }
    if (blk == t_blocks && tid == 0) {
        double t = 0.0;
        for (int g = 0; g < a.G; ++g) t += (double)a.nllp[g];
        if (a.nll_out) a.nll_out[0] = (float)t;
        if (a.cost_out) a.cost_out[0] = (float)t;
    }
}

}  // namespace

hipError_t launch_class_prep(const ClassPrepArgs& a, hipStream_t s)
{
    if (a.B < 1 || a.V < 1 || a.ldv < a.V || (a.ldv & 3) || !a.v0 || !a.xt || a.lo < 0 || a.K < 1 || a.lo + a.K > a.V ||
        (a.svp != nullptr && a.nv == nullptr) || (a.copy_nv != nullptr && a.nv == nullptr))
        return hipErrorInvalidValue;
    const unsigned gy = (unsigned)(((a.ldv >> 2) + 255) / 256);
    if (gy > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(class_prep_kernel, dim3((unsigned)class_prep_chunks(a.B), gy), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_class_forward(const ClassForwardArgs& a, hipStream_t s)
{
    const bool train = a.rpos != nullptr;
    if (a.B < 1 || a.H < 1 || a.ldh < a.H || a.K < 2 || a.K > MDBN_GROUP_MAX || a.R < 1 || a.R > CLASS_R || !a.A || !a.U || !a.d ||
        a.G < 1 || a.G > (a.B + a.R - 1) / a.R || (a.logp != nullptr && a.label == nullptr) || (a.post != nullptr && a.ldk < a.K))
        return hipErrorInvalidValue;
    if (train && (!a.rbar || !a.Tp || !a.np || !a.nllp || !a.label || (a.ph != nullptr && (!a.nh || !a.ph_out || !a.nh_out))))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(class_forward_kernel, dim3((unsigned)a.G), dim3(CLASS_NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_class_patch(const ClassPatchArgs& a, hipStream_t s)
{
    if (a.V < 1 || a.H < 1 || a.K < 2 || a.K > MDBN_GROUP_MAX || a.lo < 0 || a.lo + a.K > a.V || a.G < 1 || a.ldh < a.H || a.ldv < a.V ||
        !a.Tp || !a.np || !a.nllp || !a.S || !a.s_v || (a.svp != nullptr && a.chunks < 1))
        return hipErrorInvalidValue;
    const int h_blocks = (a.H + 255) / 256, t_blocks = a.K * h_blocks, v_blocks = (a.V + 255) / 256;
    hipLaunchKernelGGL(class_patch_kernel, dim3((unsigned)(t_blocks + v_blocks)), dim3(256), 0, s, a, h_blocks, t_blocks);
    return hipGetLastError();
}

}  // namespace mdbn

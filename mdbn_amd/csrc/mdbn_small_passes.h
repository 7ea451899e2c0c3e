// The LDS-resident passes of the one-launch kernels (mdbn_small.hip: CD-k step; mdbn_ais.hip: annealed importance sampling;
// mdbn_clamp.hip: clamped Gibbs sampling):
// D[4][N] = A[4][K] * op(W) on v_mfma_f32_4x4x1_16b_f32 with every operand in LDS.  Included by those three sources only; the
// layout and the reasons for it are described at the top of mdbn_small.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mdbn_small.h"

namespace mdbn {

typedef float sf32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t su32x4 __attribute__((ext_vector_type(4)));
// Every LDS pointer of this file carries its address space in its TYPE: held as plain `float*` (in arrays, across lambdas)
// hipcc loses track of it and emits FLAT loads -- the vector-memory path with an aperture check, several times slower than
// ds_read and counted on vmcnt (seen in the ISA: v_lshl_add_u64 pointer arithmetic and s_waitcnt vmcnt(0) in the MFMA loops).
typedef __attribute__((address_space(3))) float lds_f;
typedef __attribute__((address_space(3))) const float lds_cf;
typedef __attribute__((address_space(3))) sf32x4 lds_f4;      // 16-byte LDS accesses (float4 is a class: no address-space copy)

// The barriers of this kernel order LDS traffic only.  __syncthreads() also waits for every outstanding GLOBAL store of the
// wave (the inspection copies and chain taps each epilogue writes): ~1-2 us per barrier, 26 barriers per CD-5 slab.
#define SM_SYNC() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

namespace {

#ifdef MDBN_STAMP_CLK   // diagnostic builds (with -DMDBN_STAMP): shader-clock cycles workgroup 0 / wave 0 spends in the parts of a pass
                        // (slots 48..55); each costs a memory round trip of thread 0: the phase stamps are then ~0.1 us per part too long
__device__ unsigned long long* g_sm_clk = nullptr;
#define SM_CLK_BEGIN() const long long clk_ = clock64()
#define SM_CLK_ADD(SLOT) do { if (g_sm_clk && blockIdx.x == 0 && threadIdx.x == 0) g_sm_clk[SLOT] += (unsigned long long)(clock64() - clk_); } while (0)
#else
#define SM_CLK_BEGIN() do { } while (0)
#define SM_CLK_ADD(SLOT) do { } while (0)
#endif

#ifndef SM_RNG_WAVE
#define SM_RNG_WAVE 0       // 1: a ninth wave draws the propup epilogues' Philox blocks under the other waves' reduction loops
#endif
#ifndef SM_SUM_UNROLLED
#define SM_SUM_UNROLLED 1   // propup epilogue: all chunk partials requested at once (0: a rolled read-wait-add loop)
#endif

// 16 rank-1 updates of a 4 x 64 tile: A register `A_` (16 k-steps, one per block), B values B_(0) .. B_(15); two accumulator
// chains (even / odd k) so that an MFMA never waits for the one before it.  (abid must be an immediate: spelled out.)
#define SM_MMA1(ACC, A_, BV, U) ACC = __builtin_amdgcn_mfma_f32_4x4x1f32(A_, BV, ACC, 4, U, 0)
#define SM_MMA16(ACC0, ACC1, A_, B_)                                                                                   \
    SM_MMA1(ACC0, A_, B_(0), 0);   SM_MMA1(ACC1, A_, B_(1), 1);   SM_MMA1(ACC0, A_, B_(2), 2);   SM_MMA1(ACC1, A_, B_(3), 3);   \
    SM_MMA1(ACC0, A_, B_(4), 4);   SM_MMA1(ACC1, A_, B_(5), 5);   SM_MMA1(ACC0, A_, B_(6), 6);   SM_MMA1(ACC1, A_, B_(7), 7);   \
    SM_MMA1(ACC0, A_, B_(8), 8);   SM_MMA1(ACC1, A_, B_(9), 9);   SM_MMA1(ACC0, A_, B_(10), 10); SM_MMA1(ACC1, A_, B_(11), 11); \
    SM_MMA1(ACC0, A_, B_(12), 12); SM_MMA1(ACC1, A_, B_(13), 13); SM_MMA1(ACC0, A_, B_(14), 14); SM_MMA1(ACC1, A_, B_(15), 15)

// One pass of the chain, D[4][N] = A[4][K] * op(W), in two forms.  No operand masking anywhere: the pad columns of the
// 4-row buffers and the pad rows / columns of W's image hold exact zeros (every writer keeps them so), a lane's column index
// is clamped into the image, and a column n >= N computes something finite that `epi` discards.
//
// sm_up (propup, K = V long, N = H: one or two 64-column tiles): work items = (tile, K chunk) dealt over the waves; a lane
// reads W[k][its column] (lanes side by side: no conflicts), 16 k-steps per A register, the next group's operands in flight
// under the MFMAs of this one.  The chunk partials go through `part` as one float4 per (chunk, column); after a barrier
// thread c sums the chunks of column c in chunk order and applies `epi` ONCE.
//
// sm_down (propdown, K = H short, N = V: up to 8 tiles, one per wave): a lane reads 16 bytes of ITS row of W (its output
// column) per 4 k-steps; the wave applies `epi` to its accumulator registers.
struct UpFrag { float a; float b[16]; };

// LDW: W's LDS pitch as a compile-time constant (small_layout hands out 20 / 44 / 68 / 132 for H <= 132) -- the 16 reads of a
// group are then one base register + immediate offsets; with a run-time pitch (LDW = 0) each read costs an address add, and
// the loop is bound by its instruction count (57 instead of 34 per 16 MFMAs: 0.96 us per pass at 512 -> 40, stamped).
template <int LDW>
__device__ __forceinline__ void sm_up_loop(lds_cf* X, lds_cf* Wl, const SmallLayout& L, lds_f* part, int wave, int lane)
{
    const int bi = (lane & 3) * L.ldx + (lane >> 2);
    const int ldw = LDW ? LDW : L.ldw;
    for (int item = wave; item < L.tiles_up * L.ks_up; item += SM_NW) {
        SM_CLK_BEGIN();
        const int tile = item % L.tiles_up, ch = item / L.tiles_up;
        const int k0 = ch * L.per_up;
        const int groups = (min(L.Vp, k0 + L.per_up) - k0) >> 4;
        lds_cf* ap = X + bi + k0;
        lds_cf* bp = Wl + k0 * ldw + min(64 * tile + lane, ldw - 1);
        sf32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        auto load = [&](UpFrag& f, int g) {
            f.a = ap[16 * g];
            lds_cf* q = bp + 16 * g * ldw;
#pragma unroll
            for (int u = 0; u < 16; ++u) f.b[u] = q[u * ldw];
        };
        UpFrag f0, f1;
        load(f0, 0);
        for (int g = 0; g + 2 <= groups; g += 2) {       // (scheduling barriers: hipcc otherwise sinks each load to its first use)
            load(f1, g + 1);
            __builtin_amdgcn_sched_barrier(0);
#define SM_B(U) f0.b[U]
            SM_MMA16(acc0, acc1, f0.a, SM_B);
#undef SM_B
            __builtin_amdgcn_sched_barrier(0);
            load(f0, min(g + 2, groups - 1));
            __builtin_amdgcn_sched_barrier(0);
#define SM_B(U) f1.b[U]
            SM_MMA16(acc0, acc1, f1.a, SM_B);
#undef SM_B
            __builtin_amdgcn_sched_barrier(0);
        }
        if (groups & 1) {
#define SM_B(U) f0.b[U]
            SM_MMA16(acc0, acc1, f0.a, SM_B);
#undef SM_B
        }
        *(lds_f4*)(part + 4 * (ch * L.H64 + 64 * tile + lane)) = acc0 + acc1;
        SM_CLK_ADD(48);
    }
}

// `rng` (the ninth wave's job, under the other waves' reduction loops): the Philox blocks the epilogue will need, one per
// column, into `U` -- 10 rounds of quarter-rate multiplies are half of the epilogue's ~1 850 cycles, and they depend on
// nothing the pass computes.
template <class Rng, class Epi>
__device__ __forceinline__ void sm_up(lds_cf* X, lds_cf* Wl, const SmallLayout& L, lds_f* part, int wave, int lane, Rng&& rng, Epi&& epi)
{
    if (SM_RNG_WAVE && wave == SM_NW) rng();
    else
    switch (L.ldw) {
        case 20: sm_up_loop<20>(X, Wl, L, part, wave, lane); break;
        case 44: sm_up_loop<44>(X, Wl, L, part, wave, lane); break;
        case 68: sm_up_loop<68>(X, Wl, L, part, wave, lane); break;
        case 132: sm_up_loop<132>(X, Wl, L, part, wave, lane); break;
        default: sm_up_loop<0>(X, Wl, L, part, wave, lane); break;
    }
    { SM_CLK_BEGIN(); SM_SYNC(); SM_CLK_ADD(49); }
    SM_CLK_BEGIN();
    for (int col = threadIdx.x; col < L.H64; col += SM_NT + 64 * SM_RNG_WAVE) {
        // (four chunk partials requested at once, summed in chunk order: a rolled read-wait-add loop is an LDS round trip per
        //  chunk; chunks past ks_up re-read the last one and add an exact zero)
#if SM_SUM_UNROLLED
        sf32x4 pc[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) pc[ch] = *(const lds_f4*)(part + 4 * (min(ch, L.ks_up - 1) * L.H64 + col));
        sf32x4 x = pc[0];
#pragma unroll
        for (int ch = 1; ch < 4; ++ch) x += ch < L.ks_up ? pc[ch] : sf32x4{0.f, 0.f, 0.f, 0.f};
        if (L.ks_up > 4) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) pc[ch] = *(const lds_f4*)(part + 4 * (min(4 + ch, L.ks_up - 1) * L.H64 + col));
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) x += 4 + ch < L.ks_up ? pc[ch] : sf32x4{0.f, 0.f, 0.f, 0.f};
        }
#else
        sf32x4 x = *(const lds_f4*)(part + 4 * col);
        for (int ch = 1; ch < L.ks_up; ++ch) x += *(const lds_f4*)(part + 4 * (ch * L.H64 + col));
#endif
        epi(x, col);
    }
    SM_CLK_ADD(50);
    { SM_CLK_BEGIN(); SM_SYNC(); SM_CLK_ADD(51); }
}

template <class Epi>
__device__ __forceinline__ void sm_down(lds_cf* Hs, lds_cf* Wl, const SmallLayout& L, int wave, int lane, Epi&& epi)
{
    const int bi = (lane & 3) * L.ldhs + (lane >> 2);
    const int groups = L.Hp >> 4;
    for (int tile = wave; tile < L.tiles_dn; tile += SM_NW) {
        SM_CLK_BEGIN();
        lds_cf* ap = Hs + bi;
        const lds_f4* bp = (const lds_f4*)(Wl + min(64 * tile + lane, L.Vp - 1) * L.ldw);
        sf32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        struct Frag { float a; sf32x4 b[4]; };
        auto load = [&](Frag& f, int g) {
            f.a = ap[16 * g];
#pragma unroll
            for (int q = 0; q < 4; ++q) f.b[q] = bp[4 * g + q];
        };
        Frag f0, f1;
        load(f0, 0);
        for (int g = 0; g + 2 <= groups; g += 2) {
            load(f1, g + 1);
            __builtin_amdgcn_sched_barrier(0);
#define SM_B(U) f0.b[(U) >> 2][(U) & 3]
            SM_MMA16(acc0, acc1, f0.a, SM_B);
#undef SM_B
            __builtin_amdgcn_sched_barrier(0);
            load(f0, min(g + 2, groups - 1));
            __builtin_amdgcn_sched_barrier(0);
#define SM_B(U) f1.b[(U) >> 2][(U) & 3]
            SM_MMA16(acc0, acc1, f1.a, SM_B);
#undef SM_B
            __builtin_amdgcn_sched_barrier(0);
        }
        if (groups & 1) {
#define SM_B(U) f0.b[(U) >> 2][(U) & 3]
            SM_MMA16(acc0, acc1, f0.a, SM_B);
#undef SM_B
        }
        SM_CLK_ADD(52);
        epi(acc0 + acc1, 64 * tile + lane);
        SM_CLK_ADD(53);
    }
    { SM_CLK_BEGIN(); SM_SYNC(); SM_CLK_ADD(54); }
}

}  // namespace

}  // namespace mdbn

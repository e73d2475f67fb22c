// MFMA shape probe of the eight-wave LDS ring (the `ringnw` ring of tools/hamming_unit_probe5.hip: eight waves per workgroup, waves 0..3
// copy one K-step each, one s_barrier per tile, four waves per SIMD by amdgpu_waves_per_eu, random +-1 operands by pointer, accumulators
// started at 704 - row * 2^-14): the same 32 x 32 x 256 unit on the two fp4 shapes of v_mfma_f32_*_f8f6f4.
//   (a) 4 x 32x32x64, one chain of four on a 16-register accumulator, the 15-op block update       (probe 5's row (c), the anchor)
//   (b) 8 x 16x16x128, period of one tile: per 16-query group two chains of two on 4-register accumulators (row halves), two block
//       maxima (4 ops), med3 / max3 / max (3), two re-base adds: 9 per group, 18 per unit
//   (c) 8 x 16x16x128, period of two tiles: the chains of the pair's two tiles start 32 eps apart and the running pair is re-based
//       once per pair: 8 per group and tile, 16 per unit
//   (d) the MFMAs of (a) alone (one v_max per unit keeps the accumulator alive)
//   (e) the MFMAs of (b) alone (one v_max3 per group keeps both accumulators alive)
// The ring, the four ds_read_b128 per tile and their addresses are the same in every arm; a wave holds 128 queries in 64 registers in
// both shapes (4 tiles x 4 K-steps, or 8 groups x 2 K-halves).  Only the structure of the instruction stream is probed: the operands
// are random nibbles, no placement rule is applied.
// Two rounds with the calls alternating, behind a warm-up round that does not count; per call the in-kernel clock (shader-clock cycles
// over 100 MHz real-time ticks, summed over the waves), cycles per unit per SIMD over the launch's span, and units per second of the
// whole chip.  Arms (b), (c), (e) write their MFMAs out in the stated order and tie the running pair to its registers (see mf16_group,
// update_halves): arm (c) runs its two tiles per loop in one copy per wave role, as the library does.
// Build: hipcc -w -O3 --offload-arch=gfx950 -fno-honor-nans -o tools/bin/hamming_unit_probe6 tools/hamming_unit_probe6.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <type_traits>
#include <algorithm>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

__device__ __forceinline__ v16f mf32(uint4 a, uint4 b, v16f c) {
    const v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const v8i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, 0, 0, 0);
}
// One 16-query group of a tile: the two row halves' chains of two, interleaved as written (the compiler's scheduler puts a chain's two
// dependent MFMAs back to back); s_nop 7 is the wait it inserts itself between a 16x16x128 fp4 MFMA and a VALU read of its result.
__device__ __forceinline__ void mf16_group(const u32x4 (&a)[4], const uint4 &b0, const uint4 &b1, const v4f &ci0, const v4f &ci1, v4f &c0, v4f &c1) {
    const u32x4 q0 = {b0.x, b0.y, b0.z, b0.w}, q1 = {b1.x, b1.y, b1.z, b1.w};
    asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %2, %6, %8 cbsz:4 blgp:4\n\t"
                 "v_mfma_f32_16x16x128_f8f6f4 %1, %4, %6, %9 cbsz:4 blgp:4\n\t"
                 "v_mfma_f32_16x16x128_f8f6f4 %0, %3, %7, %0 cbsz:4 blgp:4\n\t"
                 "v_mfma_f32_16x16x128_f8f6f4 %1, %5, %7, %1 cbsz:4 blgp:4\n\t"
                 "s_nop 7"
                 : "=&v"(c0), "=&v"(c1)
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(q0), "v"(q1), "v"(ci0), "v"(ci1));
}
__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ void update4(float &m1, float &m2, float a0, float a1, float a2, float a3) {
    const float s0 = __builtin_amdgcn_fmed3f(m1, a0, a1);
    const float t0 = max3(m1, a0, a1);
    const float s1 = __builtin_amdgcn_fmed3f(t0, a2, a3);
    m1 = max3(t0, a2, a3);
    m2 = max3(m2, s0, s1);
}
// maxima of four groups of four candidates (8 ops), one update4 over them (5), two re-base adds: the 15-op update of the library
__device__ __forceinline__ void update_blocks4(float &m1r, float &m2r, const v16f &acc) {
    float m1 = m1r + 0.001953125f, m2 = m2r + 0.001953125f;
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = __builtin_fmaxf(max3(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2]), acc[4 * j + 3]);
    update4(m1, m2, g[0], g[1], g[2], g[3]);
    m1r = m1, m2r = m2;
}
// the two block maxima of a group's row halves (4 ops) and the fold into the running pair (3): 7 ops, then REBASE re-base adds (0 | 2).
// The fold is written out with the running pair tied to its registers: left to the compiler the two tiles' folds of a pair become one
// v_max3 over both tiles' `s`, the re-base adds pair up into v_pk_add_f32 over neighbouring groups, and the renamed copies and aligned
// pairs this needs push the two-tile body over 128 VGPRs.
template <int REBASE>
__device__ __forceinline__ void update_halves(float &m1, float &m2, const v4f &c0, const v4f &c1, float step) {
    const float g0 = __builtin_fmaxf(max3(c0[0], c0[1], c0[2]), c0[3]);
    const float g1 = __builtin_fmaxf(max3(c1[0], c1[1], c1[2]), c1[3]);
    float s;
    if constexpr (REBASE)
        asm volatile("v_med3_f32 %2, %0, %3, %4\n\tv_max3_f32 %0, %0, %3, %4\n\tv_max_f32 %1, %1, %2\n\tv_add_f32 %0, %5, %0\n\tv_add_f32 %1, %5, %1"
                     : "+v"(m1), "+v"(m2), "=&v"(s) : "v"(g0), "v"(g1), "s"(step));
    else
        asm volatile("v_med3_f32 %2, %0, %3, %4\n\tv_max3_f32 %0, %0, %3, %4\n\tv_max_f32 %1, %1, %2" : "+v"(m1), "+v"(m2), "=&v"(s) : "v"(g0), "v"(g1));
}

enum { ARM_A = 0, ARM_B = 1, ARM_C = 2, ARM_D = 3, ARM_E = 4 };
constexpr int QT = 4, NG = 2 * QT, NW = 8, WPE = 4, NBS = 4;
constexpr int kSrcU4 = 64 * 64;   // operand buffer: 8 stages of 256 uint4 (train) and the query fragments behind the first stage
constexpr float kEps = 1.0f / 16384.0f;

// iters is even: arm (c) runs pairs of tiles
template <int ARM>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void ringnw(const uint4 *__restrict__ src, float bias, float *out, int iters,
                                                                                                  long long *cyc) {
    constexpr bool S16 = ARM == ARM_B || ARM == ARM_C || ARM == ARM_E;
    __shared__ __attribute__((aligned(16))) uint4 ring[NBS][256];
    for (int i = threadIdx.x; i < NBS * 256; i += 64 * NW) ring[i >> 8][i & 255] = src[i & 255];
    __syncthreads();
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint4 b[4 * QT];   // 32 shape: [tile][K-step]; 16 shape: [group][K-half]
    for (int i = 0; i < 4 * QT; ++i) b[i] = src[l + 64 * (4 + i)];   // (<= 64 * 19 + 63 < kSrcU4)
    v16f cinit32;
    for (int i = 0; i < 16; ++i) cinit32[i] = bias - (float)i * kEps;
    // 16 shape: a lane's registers of row half rh are rows 16 rh + 4 (l >> 4) + i; tile J = 0 of a pair starts 32 eps higher
    v4f cinit16[2][2];
    for (int J = 0; J < 2; ++J)
        for (int rh = 0; rh < 2; ++rh)
            for (int i = 0; i < 4; ++i)
                cinit16[J][rh][i] = bias + (float)((ARM == ARM_C && J == 0 ? 32 : 0) - (16 * rh + 4 * (l >> 4) + i)) * kEps;
    float m1[NG], m2[NG];
    for (int t = 0; t < NG; ++t) m1[t] = m2[t] = -1e30f;
    const uint4 *tbase = src + (size_t)(w & 3) * 64;
    auto copy_stage = [&](int st) {   // (reads src[(st & 7) * 256 + (w & 3) * 64 + l] <= 2047 < kSrcU4)
        if (w < 4)
            __builtin_amdgcn_global_load_lds((const void *)(tbase + (size_t)((st & 7) * 256) + l),
                                             (__attribute__((address_space(3))) void *)&ring[st & (NBS - 1)][w * 64], 16, 0, 0);
    };
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0] + (uint32_t)l * 16u;
    // one tile: copy two ahead, barrier, four ds_read_b128, the unit of the arm for the wave's 128 queries
    // role: 0 = the wave tests its role in the loop (probe 5's stream), 1 = copier, -1 = consumer
    auto tile = [&](int st, int J, auto role) {
        constexpr int R = decltype(role)::value;
        if constexpr (ARM == ARM_C) __builtin_amdgcn_sched_barrier(0);   // (a tile's instructions stay inside the tile, as a back edge keeps them)
        if constexpr (R >= 0) copy_stage(st + 2);
        if constexpr (R == 0) {
            if (w < 4) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else if constexpr (R > 0) {
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        u32x4 r[4];
        const uint32_t addr = ring_lds + (uint32_t)(st & (NBS - 1)) * 4096u;
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072"
                     : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]) : "v"(addr) : "memory");
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[0]));
        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[1]));
        asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[2]));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[3]));
        uint4 a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = make_uint4(r[s].x, r[s].y, r[s].z, r[s].w);
        if constexpr (!S16) {
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                v16f acc = mf32(a[0], b[4 * t], cinit32);
#pragma unroll
                for (int s = 1; s < 4; ++s) acc = mf32(a[s], b[4 * t + s], acc);
                if constexpr (ARM == ARM_A)
                    update_blocks4(m1[t], m2[t], acc);
                else
                    m1[t] = __builtin_fmaxf(m1[t], acc[0]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NG; ++u) {
                v4f c0, c1;
                mf16_group(r, b[2 * u], b[2 * u + 1], cinit16[J][0], cinit16[J][1], c0, c1);
                if constexpr (ARM == ARM_E) {
                    m1[u] = max3(m1[u], c0[0], c1[0]);
                } else {
                    // (b) re-bases by 32 eps per tile, (c) by 64 eps per pair after its second tile
                    if (ARM == ARM_B || J == 1) update_halves<1>(m1[u], m2[u], c0, c1, (ARM == ARM_B ? 32.0f : 64.0f) * kEps);
                    else update_halves<0>(m1[u], m2[u], c0, c1, 0.0f);
                }
                __builtin_amdgcn_sched_barrier(0);   // (one (c0, c1) pair alive at a time: left alone the scheduler interleaves the groups and spills)
            }
        }
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    copy_stage(0);
    copy_stage(1);
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    if constexpr (ARM == ARM_C) {
        // one copy of the loop per role, as in the library: with the role tested inside the two-tile body the updates of a tile sink past
        // the branch, all eight groups' accumulators stay alive and the body spills
        auto run_pairs = [&](auto role) {
            for (int st = 0; st < iters; st += 2) {
                tile(st, 0, role);
                tile(st + 1, 1, role);
            }
        };
        if (w < 4) run_pairs(std::integral_constant<int, 1>{});
        else run_pairs(std::integral_constant<int, -1>{});
    } else {
        for (int st = 0; st < iters; ++st) tile(st, 1, std::integral_constant<int, 0>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const int wv = blockIdx.x * NW + (threadIdx.x >> 6);   // (< blocks * NW = the records allocated)
        cyc[4 * wv] = t1 - t0, cyc[4 * wv + 1] = r1 - r0, cyc[4 * wv + 2] = r0, cyc[4 * wv + 3] = r1;
    }
    float sres = 0.f;
    for (int t = 0; t < (S16 ? NG : QT); ++t) sres += m1[t] + m2[t];
    out[(blockIdx.x * blockDim.x + threadIdx.x) & 16383] = sres;
}

template <int ARM>
void run(const char *name, const uint4 *src, float bias, float *out, int cus, int round) {
    long long *dc;
    const int blocks = cus * WPE * 4 / NW, waves = blocks * NW, iters = 3000;
    CHECK(hipMalloc(&dc, (size_t)waves * 32));
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(ringnw<ARM>, dim3(blocks), dim3(64 * NW), 0, 0, src, bias, out, iters, dc);
    CHECK(hipGetLastError());
    std::vector<long long> h((size_t)waves * 4);
    CHECK(hipMemcpy(h.data(), dc, (size_t)waves * 32, hipMemcpyDeviceToHost));
    double cs = 0, rs = 0;
    long long rmin = h[2], rmax = h[3];
    for (int i = 0; i < waves; ++i) {
        cs += h[4 * i], rs += h[4 * i + 1];
        rmin = std::min(rmin, h[4 * i + 2]);
        rmax = std::max(rmax, h[4 * i + 3]);
    }
    const double ghz = cs / rs * 0.1, span_s = (double)(rmax - rmin) * 1e-8;
    const double units = (double)waves * iters * QT;
    printf("round %d  %-52s %.3f GHz  %6.1f cycles per unit per SIMD  %.4e units/s\n", round, name, ghz,
           (double)(rmax - rmin) * (cs / rs) / (iters * (double)QT * WPE), units / span_s);
    fflush(stdout);
    CHECK(hipFree(dc));
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    uint4 *rnd;
    float *out;
    CHECK(hipMalloc(&rnd, kSrcU4 * 16));
    CHECK(hipMalloc(&out, 16384 * 4));
    std::vector<uint32_t> h(kSrcU4 * 4);
    uint32_t x = 12345;
    for (auto &v : h) {
        uint32_t w = 0;
        for (int k = 0; k < 8; ++k) {
            x = x * 1664525u + 1013904223u;
            w |= ((x >> 16) & 1 ? 0x2u : 0xAu) << (4 * k);
        }
        v = w;
    }
    CHECK(hipMemcpy(rnd, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    const float bias = 704.0f;
    printf("%d CUs, ringnw 128 queries per wave, waves/workgroup=%d waves/SIMD=%d, random operands, C = %.0f - row eps\n", cus, NW, WPE, bias);
    // the first launches of a process run at a clock of their own (1.66-1.75 GHz in the first row of probe 5) and the clock keeps rising
    // through the first ten calls: round -1 is a warm-up and does not count
    for (int round = -1; round < 2; ++round) {
        run<ARM_A>("(a) 4 x 32x32x64, 15-op block update", rnd, bias, out, cus, round);
        run<ARM_B>("(b) 8 x 16x16x128, period of one tile, 18 ops", rnd, bias, out, cus, round);
        run<ARM_C>("(c) 8 x 16x16x128, period of two tiles, 16 ops", rnd, bias, out, cus, round);
        run<ARM_D>("(d) 4 x 32x32x64, MFMAs only", rnd, bias, out, cus, round);
        run<ARM_E>("(e) 8 x 16x16x128, MFMAs only", rnd, bias, out, cus, round);
    }
    CHECK(hipDeviceSynchronize());
    return 0;
}

// Vector-issue probe of the 16x16x128 unit of the eight-wave LDS ring: arm (c) of tools/hamming_unit_probe6.hip (eight waves per workgroup, waves
// 0..3 copy one K-step each, one s_barrier per tile, four waves per SIMD, random +-1 operands, accumulators started at 704 - row * 2^-14, two
// tiles per loop in one copy per wave role) EXTENDED by the in-kernel expansion of the library's kernel: per tile every wave issues one
// ds_read_b32 of a raw word, the plane ops (v_bfe, shift, two and / v_lshl_or) and one ds_write_b64, so that the unit's vector-op count is the
// kernel's.  (The planes go to an LDS area of their own: the ring protocol of probe 6 stays as it is, only the instruction stream is probed.)
// Per 32 x 32 unit a wave issues 8 MFMAs of 16 cycles (64 cycles of vector issue out of 128) plus
//   (a) today's update: two block maxima of four (4 ops), med3 / max3 / max (3), two re-base adds per pair of tiles       16 ops per unit
//   (b) absolute-row C: C = 704 - (32 t + lr) eps advanced by four v_pk_add_f32 per tile and wave, no re-base             15
//   (c) block of eight: three v_max3 and a v_max, med3 / max (6), two re-base adds per pair of tiles                      14
//   (d) both                                                                                                              13
// plus ~1.5 ops per unit of expansion in every arm.  Two rounds with the calls alternating behind a warm-up round that does not count; per call
// the in-kernel clock, cycles per unit per SIMD over the launch's span, and units per second of the whole chip.
// Build: hipcc -w -O3 --offload-arch=gfx950 -fno-honor-nans -o tools/bin/hamming_unit_probe7 tools/hamming_unit_probe7.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <type_traits>
#include <algorithm>
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

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
// BLOCK8 = 0: two block maxima of four and med3 / max3 / max; 1: one maximum of eight and med3 / max.  REBASE: two adds first.
template <int BLOCK8, int REBASE>
__device__ __forceinline__ void update(float &m1, float &m2, const v4f &c0, const v4f &c1, float step) {
    if constexpr (BLOCK8) {
        float g = max3(c0[0], c0[1], c0[2]);
        g = max3(g, c0[3], c1[0]);
        g = max3(g, c1[1], c1[2]);
        g = __builtin_fmaxf(g, c1[3]);
        if constexpr (REBASE)
            asm volatile("v_add_f32 %0, %3, %0\n\tv_add_f32 %1, %3, %1\n\tv_med3_f32 %1, %0, %1, %2\n\tv_max_f32 %0, %0, %2" : "+v"(m1), "+v"(m2) : "v"(g), "s"(step));
        else
            asm volatile("v_med3_f32 %1, %0, %1, %2\n\tv_max_f32 %0, %0, %2" : "+v"(m1), "+v"(m2) : "v"(g));
    } else {
        const float g0 = __builtin_fmaxf(max3(c0[0], c0[1], c0[2]), c0[3]);
        const float g1 = __builtin_fmaxf(max3(c1[0], c1[1], c1[2]), c1[3]);
        float s;
        if constexpr (REBASE)
            asm volatile("v_add_f32 %0, %5, %0\n\tv_add_f32 %1, %5, %1\n\tv_med3_f32 %2, %0, %3, %4\n\tv_max3_f32 %0, %0, %3, %4\n\tv_max_f32 %1, %1, %2"
                         : "+v"(m1), "+v"(m2), "=&v"(s) : "v"(g0), "v"(g1), "s"(step));
        else
            asm volatile("v_med3_f32 %2, %0, %3, %4\n\tv_max3_f32 %0, %0, %3, %4\n\tv_max_f32 %1, %1, %2" : "+v"(m1), "+v"(m2), "=&v"(s) : "v"(g0), "v"(g1));
    }
}

constexpr int QT = 4, NG = 2 * QT, NW = 8, WPE = 4, NBS = 4;
constexpr int kSrcU4 = 64 * 64;   // operand buffer: 8 stages of 256 uint4 (train) and the query fragments behind the first stage
constexpr float kEps = 1.0f / 16384.0f;

// ABS = absolute-row C, BLOCK8 = block of eight; iters is even
template <int ABS, int BLOCK8>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void ringnw(const uint4 *__restrict__ src, float bias, float *out, int iters,
                                                                                                  long long *cyc) {
    __shared__ __attribute__((aligned(16))) uint4 ring[NBS][256];
    __shared__ __attribute__((aligned(16))) uint32_t raw[4 * 256];       // raw words the expansion reads (never rewritten: random bits)
    __shared__ __attribute__((aligned(16))) uint32_t planes[2][NW * 128];   // where it writes: 8 bytes per lane and wave, two slots
    for (int i = threadIdx.x; i < NBS * 256; i += 64 * NW) ring[i >> 8][i & 255] = src[i & 255];
    for (int i = threadIdx.x; i < 4 * 256; i += 64 * NW) raw[i] = src[i].x;
    __syncthreads();
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint4 b[4 * QT];   // [group][K-half]
    for (int i = 0; i < 4 * QT; ++i) b[i] = src[l + 64 * (4 + i)];   // (<= 64 * 19 + 63 < kSrcU4)
    // a lane's registers of row half rh are rows 16 rh + 4 (l >> 4) + i; without ABS tile J = 0 of a pair starts 32 eps higher
    v4f cinit16[2][2];
    for (int J = 0; J < 2; ++J)
        for (int rh = 0; rh < 2; ++rh)
            for (int i = 0; i < 4; ++i) cinit16[J][rh][i] = bias + (float)((!ABS && J == 0 ? 32 : 0) - (16 * rh + 4 * (l >> 4) + i)) * kEps;
    v2f pk_step = {-32.0f * kEps, -32.0f * kEps};
    asm volatile("" : "+s"(pk_step));
    float m1[NG], m2[NG];
    for (int t = 0; t < NG; ++t) m1[t] = m2[t] = -1e30f;
    const uint4 *tbase = src + (size_t)(w & 3) * 64;
    auto copy_stage = [&](int st) {   // (reads src[(st & 7) * 256 + (w & 3) * 64 + l] <= 2047 < kSrcU4)
        if (w < 4)
            __builtin_amdgcn_global_load_lds((const void *)(tbase + (size_t)((st & 7) * 256) + l),
                                             (__attribute__((address_space(3))) void *)&ring[st & (NBS - 1)][w * 64], 16, 0, 0);
    };
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0] + (uint32_t)l * 16u;
    // the library's addresses: raw word w of row l >> 1 (bytes 0 .. 2047 of a 4 KiB area), plane pair l & 1 in bit 3 of the write address
    uint32_t xp_raw = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&raw[0] + (uint32_t)w * 4u + (uint32_t)(l >> 1) * 32u;
    uint32_t xp_plane = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&planes[0][0] + (uint32_t)w * 512u + (uint32_t)l * 8u;
    asm volatile("" : "+v"(xp_raw), "+v"(xp_plane));
    auto tile = [&](int st, auto jc, auto role) {
        constexpr int R = decltype(role)::value, J = decltype(jc)::value;
        __builtin_amdgcn_sched_barrier(0);   // (a tile's instructions stay inside the tile, as a back edge keeps them)
        if constexpr (R > 0) {
            copy_stage(st + 2);
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        u32x4 r[4];
        uint32_t x;
        const uint32_t addr = ring_lds + (uint32_t)(st & (NBS - 1)) * 4096u;
        asm volatile("ds_read_b32 %4, %6 offset:%7\n\tds_read_b128 %0, %5\n\tds_read_b128 %1, %5 offset:1024\n\tds_read_b128 %2, %5 offset:2048\n\t"
                     "ds_read_b128 %3, %5 offset:3072"
                     : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(x) : "v"(addr), "v"(xp_raw), "i"(J * 2048) : "memory");
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x));
        {
            const uint32_t y = x >> __builtin_amdgcn_ubfe(xp_plane, 3u, 1u);
            u32x2 o;
            asm("v_lshl_or_b32 %0, %1, 3, %2" : "=v"(o.x) : "v"(y & 0x11111111u), "s"(0x22222222u));
            asm("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(o.y) : "v"(y & 0x44444444u), "s"(0x22222222u));
            asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(xp_plane), "v"(o), "i"(((J + 1) & 1) * (NW * 512)) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(r[0]));
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[1]));
        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[2]));
        asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[3]));
        v4f(&c)[2] = cinit16[ABS ? 0 : J];
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            v4f c0, c1;
            mf16_group(r, b[2 * u], b[2 * u + 1], c[0], c[1], c0, c1);
            if constexpr (!ABS && J == 1) update<BLOCK8, 1>(m1[u], m2[u], c0, c1, 64.0f * kEps);
            else update<BLOCK8, 0>(m1[u], m2[u], c0, c1, 0.0f);
            __builtin_amdgcn_sched_barrier(0);   // (one (c0, c1) pair alive at a time)
        }
        if constexpr (ABS) {
            const v2f stp = pk_step;
            asm volatile("v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %2" : "+v"(c[0].lo), "+v"(c[0].hi) : "s"(stp));
            asm volatile("v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %2" : "+v"(c[1].lo), "+v"(c[1].hi) : "s"(stp));
        }
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    copy_stage(0);
    copy_stage(1);
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    auto run_pairs = [&](auto role) {
        // splits of 256 tiles, as a train set of 8192 rows has them: C starts again at row 0 (ABS; 8 adds per 256 tiles)
        for (int s0 = 0; s0 < iters; s0 += 256) {
            const int s1 = min(iters, s0 + 256);
#pragma unroll 1
            for (int st = s0; st < s1; st += 2) {
                tile(st, std::integral_constant<int, 0>{}, role);
                tile(st + 1, std::integral_constant<int, 1>{}, role);
            }
            if constexpr (ABS)
                for (int rh = 0; rh < 2; ++rh)
                    for (int i = 0; i < 4; ++i) cinit16[0][rh][i] += (float)(32 * (s1 - s0)) * kEps;
        }
    };
    if (w < 4) run_pairs(std::integral_constant<int, 1>{});
    else run_pairs(std::integral_constant<int, -1>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const int wv = blockIdx.x * NW + (threadIdx.x >> 6);   // (< blocks * NW = the records allocated)
        cyc[4 * wv] = t1 - t0, cyc[4 * wv + 1] = r1 - r0, cyc[4 * wv + 2] = r0, cyc[4 * wv + 3] = r1;
    }
    float sres = planes[0][threadIdx.x] + planes[1][threadIdx.x];
    for (int t = 0; t < NG; ++t) sres += m1[t] + m2[t];
    out[(blockIdx.x * blockDim.x + threadIdx.x) & 16383] = sres;
}

template <int ABS, int BLOCK8>
void run(const char *name, const uint4 *src, float bias, float *out, int cus, int round) {
    long long *dc;
    const int blocks = cus * WPE * 4 / NW, waves = blocks * NW, iters = 3000;
    CHECK(hipMalloc(&dc, (size_t)waves * 32));
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((ringnw<ABS, BLOCK8>), dim3(blocks), dim3(64 * NW), 0, 0, src, bias, out, iters, dc);
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
    printf("%d CUs, ringnw 128 queries per wave with in-kernel expansion, waves/workgroup=%d waves/SIMD=%d, random operands, C = %.0f - row eps\n", cus, NW, WPE, bias);
    for (int round = -1; round < 2; ++round) {   // (round -1 is a warm-up and does not count)
        run<0, 0>("(a) two block maxima of four, re-base per pair, 16 ops", rnd, bias, out, cus, round);
        run<1, 0>("(b) absolute-row C, 15 ops", rnd, bias, out, cus, round);
        run<0, 1>("(c) block of eight, re-base per pair, 14 ops", rnd, bias, out, cus, round);
        run<1, 1>("(d) absolute-row C and block of eight, 13 ops", rnd, bias, out, cus, round);
    }
    CHECK(hipDeviceSynchronize());
    return 0;
}

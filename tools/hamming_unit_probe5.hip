// Clock attribution probe of the eight-wave LDS ring (the `ringnw` stream of tools/hamming_unit_probe4.hip with the block update of four,
// UPD = 4: eight waves per workgroup, waves 0..3 copy one K-step each, one s_barrier per tile, four waves per SIMD by amdgpu_waves_per_eu).
// The launch is power-limited: the sustained shader clock depends on how many bits switch per cycle.  The SAME instruction
// stream runs on different data, so that a clock difference belongs to the data alone:
//   (a) random +-1 operands, C = -row * 2^-14               the accumulators wander around zero: sign, exponent and the aligned mantissa
//                                                            change from one register write to the next
//   (b) random +-1 operands, C = 640 - row * 2^-14          the accumulators stay inside one binade: sign and exponent never change, the
//   (c) random +-1 operands, C = 704 - row * 2^-14          row fraction keeps its place, only the integer part's 7-9 bits move
//   (d) all-zero descriptors (every nibble 0xA = -1.0)      nothing switches from unit to unit: the ceiling
//   (e) all-zero operand words (every nibble +0.0)          the same with zero multiplier inputs (accumulator = C for ever)
// The bias is a kernel argument and the operands are a pointer: one kernel, one code object, five calls.  (b), (c) against (a) say how much
// of the distance to (d) the accumulators own.
// Per call, two rounds with the calls alternating: the in-kernel clock (shader-clock cycles over 100 MHz real-time ticks, summed over the
// waves), cycles per unit per SIMD over the launch's span, and units per second of the whole chip.
// unit = one 32 x 32 distance tile (K = 256): 4 x v_mfma_f32_32x32x64_f8f6f4 (fp4) + the 15-op update per query tile.
// Build: hipcc -w -O3 --offload-arch=gfx950 -fno-honor-nans -o tools/bin/hamming_unit_probe5 tools/hamming_unit_probe5.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <algorithm>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

__device__ __forceinline__ v16f mf(uint4 a, uint4 b, v16f c) {
    const v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const v8i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, 0, 0, 0);
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

constexpr int QT = 4, NW = 8, WPE = 4, NBS = 4;
constexpr int kSrcU4 = 64 * 64;   // operand buffer: 8 stages of 256 uint4 (train) and the query fragments behind the first stage

__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void ringnw(const uint4 *__restrict__ src, float bias, float *out, int iters,
                                                                                                  long long *cyc) {
    __shared__ __attribute__((aligned(16))) uint4 ring[NBS][256];
    for (int i = threadIdx.x; i < NBS * 256; i += 64 * NW) ring[i >> 8][i & 255] = src[i & 255];
    __syncthreads();
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint4 b[QT][4];
    for (int t = 0; t < QT; ++t)
        for (int s = 0; s < 4; ++s) b[t][s] = src[l + 64 * (4 + 4 * t + s)];   // (<= 64 * 23 + 63 < kSrcU4)
    v16f cinit;
    for (int i = 0; i < 16; ++i) cinit[i] = bias - (float)i * (1.0f / 16384.0f);
    float m1[QT], m2[QT];
    for (int t = 0; t < QT; ++t) m1[t] = m2[t] = -1e30f;
    const uint4 *tbase = src + (size_t)(w & 3) * 64;
    auto copy_stage = [&](int st) {   // (reads src[(st & 7) * 256 + (w & 3) * 64 + l] <= 2047 < kSrcU4)
        if (w < 4)
            __builtin_amdgcn_global_load_lds((const void *)(tbase + (size_t)((st & 7) * 256) + l),
                                             (__attribute__((address_space(3))) void *)&ring[st & (NBS - 1)][w * 64], 16, 0, 0);
    };
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0] + (uint32_t)l * 16u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    copy_stage(0);
    copy_stage(1);
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int st = 0; st < iters; ++st) {
        copy_stage(st + 2);
        if (w < 4) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
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
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            v16f acc = mf(a[0], b[t][0], cinit);
#pragma unroll
            for (int s = 1; s < 4; ++s) acc = mf(a[s], b[t][s], acc);
            update_blocks4(m1[t], m2[t], acc);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const int wv = blockIdx.x * NW + (threadIdx.x >> 6);   // (< blocks * NW = the records allocated)
        cyc[4 * wv] = t1 - t0, cyc[4 * wv + 1] = r1 - r0, cyc[4 * wv + 2] = r0, cyc[4 * wv + 3] = r1;
    }
    float sres = 0.f;
    for (int t = 0; t < QT; ++t) sres += m1[t] + m2[t];
    out[(blockIdx.x * blockDim.x + threadIdx.x) & 16383] = sres;
}

void run(const char *name, const uint4 *src, float bias, float *out, int cus, int round) {
    long long *dc;
    const int blocks = cus * WPE * 4 / NW, waves = blocks * NW, iters = 3000;
    CHECK(hipMalloc(&dc, (size_t)waves * 32));
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(ringnw, dim3(blocks), dim3(64 * NW), 0, 0, src, bias, out, iters, dc);
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
    printf("round %d  %-44s %.3f GHz  %6.1f cycles per unit per SIMD  %.4e units/s\n", round, name, ghz,
           (double)(rmax - rmin) * (cs / rs) / (iters * (double)QT * WPE), units / span_s);
    fflush(stdout);
    CHECK(hipFree(dc));
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    uint4 *rnd, *zero_desc, *zero_words;
    float *out;
    CHECK(hipMalloc(&rnd, kSrcU4 * 16));
    CHECK(hipMalloc(&zero_desc, kSrcU4 * 16));
    CHECK(hipMalloc(&zero_words, kSrcU4 * 16));
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
    std::fill(h.begin(), h.end(), 0xAAAAAAAAu);
    CHECK(hipMemcpy(zero_desc, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(zero_words, 0, kSrcU4 * 16));
    printf("%d CUs, ringnw QT=%d waves/workgroup=%d waves/SIMD=%d, block update of four\n", cus, QT, NW, WPE);
    for (int round = 0; round < 2; ++round) {
        run("(a) random operands, C = -row eps", rnd, 0.0f, out, cus, round);
        run("(b) random operands, C = 640 - row eps", rnd, 640.0f, out, cus, round);
        run("(c) random operands, C = 704 - row eps", rnd, 704.0f, out, cus, round);
        run("(d) all-zero descriptors (nibbles 0xA)", zero_desc, 0.0f, out, cus, round);
        run("(e) all-zero operand words (nibbles 0x0)", zero_words, 0.0f, out, cus, round);
    }
    CHECK(hipDeviceSynchronize());
    return 0;
}

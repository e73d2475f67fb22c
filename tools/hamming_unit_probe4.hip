// Unit-cost probe of the BLOCK forms of the running top-2 (option hamming_block_top2 of knn_hamming_mfma.hip), beside the per-candidate
// update: the LDS ring of tools/hamming_unit_probe3.hip (`ringnw`: eight waves per workgroup, waves 0..3 copy one K-step each, one
// s_barrier per tile, four waves per SIMD by amdgpu_waves_per_eu) with the update as a template parameter:
//   UPD = -1  MFMAs only (one v_max per unit keeps the accumulator alive)
//   UPD = 0   the 22-op update: 4 x top2_update4 + two re-base adds
//   UPD = 4   maxima of four groups of four candidates (8 ops), one top2_update4 over them (5), two adds: 15
//   UPD = 16  seven max3 reduce the 16 candidates to x, y; med3 / max3 / max fold them (3), two adds: 12
// unit = one 32 x 32 distance tile (K = 256): 4 x v_mfma_f32_32x32x64_f8f6f4 (fp4) + the update per query tile.
// Build: hipcc -w -O3 --offload-arch=gfx950 -fno-honor-nans -o tools/bin/hamming_unit_probe4 tools/hamming_unit_probe4.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <algorithm>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

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
template <int UPD>
__device__ __forceinline__ void update(float &m1r, float &m2r, const v16f &acc) {
    if constexpr (UPD < 0) {
        m1r = __builtin_fmaxf(m1r, acc[0]);
        return;
    }
    float m1 = m1r + 0.001953125f, m2 = m2r + 0.001953125f;
    if constexpr (UPD == 0) {
#pragma unroll
        for (int reg = 0; reg < 16; reg += 4) update4(m1, m2, acc[reg], acc[reg + 1], acc[reg + 2], acc[reg + 3]);
    } else if constexpr (UPD == 4) {
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = __builtin_fmaxf(max3(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2]), acc[4 * j + 3]);
        update4(m1, m2, g[0], g[1], g[2], g[3]);
    } else {
        const float p0 = max3(acc[0], acc[1], acc[2]), p1 = max3(acc[3], acc[4], acc[5]), p2 = max3(acc[6], acc[7], acc[8]);
        const float p3 = max3(acc[9], acc[10], acc[11]), p4 = max3(acc[12], acc[13], acc[14]);
        const float x = max3(p0, p1, p2), y = max3(p3, p4, acc[15]);
        const float s = __builtin_amdgcn_fmed3f(m1, x, y);
        m1 = max3(m1, x, y);
        m2 = __builtin_fmaxf(m2, s);
    }
    m1r = m1, m2r = m2;
}

template <int QT, int NW, int WPE, int UPD>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void ringnw(const uint4 *__restrict__ src, float *out, int iters, long long *cyc) {
    constexpr int NBS = 4;
    __shared__ __attribute__((aligned(16))) uint4 ring[NBS][256];
    for (int i = threadIdx.x; i < NBS * 256; i += 64 * NW) ring[i >> 8][i & 255] = src[i & 255];
    __syncthreads();
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint4 b[QT][4];
    for (int t = 0; t < QT; ++t)
        for (int s = 0; s < 4; ++s) b[t][s] = src[l + 64 * (4 + 4 * t + s)];
    v16f cinit;
    for (int i = 0; i < 16; ++i) cinit[i] = -(float)i * (1.0f / 16384.0f);
    float m1[QT], m2[QT];
    for (int t = 0; t < QT; ++t) m1[t] = m2[t] = -1e30f;
    const uint4 *tbase = src + (size_t)(w & 3) * 64;
    auto copy_stage = [&](int st) {
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
            update<UPD>(m1[t], m2[t], acc);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const int wv = blockIdx.x * NW + (threadIdx.x >> 6);
        cyc[4 * wv] = t1 - t0, cyc[4 * wv + 1] = r1 - r0, cyc[4 * wv + 2] = r0, cyc[4 * wv + 3] = r1;
    }
    float sres = 0.f;
    for (int t = 0; t < QT; ++t) sres += m1[t] + m2[t];
    out[(blockIdx.x * blockDim.x + threadIdx.x) & 16383] = sres;
}
template <int QT, int NW, int WPE, int UPD>
void run_ringnw(const uint4 *src, float *out) {
    long long *dc;
    const int blocks = 256 * WPE * 4 / NW, waves = blocks * NW, iters = 3000;
    hipMalloc(&dc, waves * 32);
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((ringnw<QT, NW, WPE, UPD>), dim3(blocks), dim3(64 * NW), 0, 0, src, out, iters, dc);
    std::vector<long long> h(waves * 4);
    hipMemcpy(h.data(), dc, waves * 32, hipMemcpyDeviceToHost);
    double cs = 0, rs = 0;
    long long rmin = h[2], rmax = h[3];
    for (int i = 0; i < waves; ++i) {
        cs += h[4 * i], rs += h[4 * i + 1];
        rmin = std::min(rmin, h[4 * i + 2]);
        rmax = std::max(rmax, h[4 * i + 3]);
    }
    const double span_cycles = (double)(rmax - rmin) * (cs / rs);
    printf("ringnw: QT=%d waves/workgroup=%d waves/SIMD=%d update=%d: %.3f GHz -> %.1f cycles per unit per SIMD (AGGREGATE), %.1f ns per unit\n", QT, NW, WPE,
           UPD, cs / rs * 0.1, span_cycles / (iters * (double)QT * WPE), (double)(rmax - rmin) * 10.0 / (iters * (double)QT * WPE));
    hipFree(dc);
}

int main() {
    uint4 *src;
    float *out;
    hipMalloc(&src, 64 * 64 * 16);
    hipMalloc(&out, 16384 * 4);
    std::vector<uint32_t> h(64 * 64 * 4);
    uint32_t x = 12345;
    for (auto &v : h) {
        uint32_t w = 0;
        for (int k = 0; k < 8; ++k) {
            x = x * 1664525u + 1013904223u;
            w |= ((x >> 16) & 1 ? 0x2u : 0xAu) << (4 * k);
        }
        v = w;
    }
    hipMemcpy(src, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    for (int round = 0; round < 2; ++round) {
        run_ringnw<4, 8, 4, -1>(src, out);
        run_ringnw<4, 8, 4, 0>(src, out);
        run_ringnw<4, 8, 4, 4>(src, out);
        run_ringnw<4, 8, 4, 16>(src, out);
    }
    hipDeviceSynchronize();
    return 0;
}

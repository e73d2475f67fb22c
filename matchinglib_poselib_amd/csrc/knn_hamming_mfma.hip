// knn_hamming_mfma.hip -- exact brute-force 2-NN under bit-Hamming distance on the gfx950 matrix cores.
//
// Same contract as knn_hamming.hip (cvflann::Index<HammingLUT>(LinearIndexParams).knnSearch of
// matchinglib/source/matchers.cpp:567-588: the two lexicographically smallest (distance, trainIdx) pairs per query,
// bit-exact), different arithmetic: every descriptor bit b becomes the fp4 (E2M1) value 2b-1 in {-1,+1}, so that
//     sum_k a'_k b'_k = (#equal bits) - (#different bits) = nbits - 2 * hamming(a, b),
// an all-pairs distance table is a dense +-1 GEMM, and v_mfma_scale_f32_32x32x64_f8f6f4 (fp4 x fp4, unit scales, fp32
// accumulate) produces 32x32 of them per K=64 step.  All sums are small integers: exact in fp32.
//
// The VALU kernels of knn_hamming.hip spend 2*NW+3 issue slots per descriptor pair (76 cycles per 64 pairs at NW = 8,
// measured issue floor); here a pair costs KS/1024 MFMAs plus TWO vector instructions:
//   * queries sit on the lanes (B operand, column = lane & 31), a 32-row train tile is the A operand, so after the K loop
//     a lane holds 16 distances of ITS query to 16 train rows;
//   * the row index rides in the accumulator: the first MFMA of a tile reads C = -(local row) * 2^-14 from 16 constant
//     registers, so v = (nbits - 2 d) - row * eps orders candidates by (distance asc, row asc) as a plain float, and the
//     running top-2 per lane is  m2 = med3(m1, m2, v); m1 = max(m1, v)  -- two VALU ops per pair, no key packing;
//   * between tiles the running pair is re-based by +32 eps (two adds per 512 pairs) instead of re-building the 16
//     constants; values stay exactly representable (|int| <= 512, fraction a multiple of 2^-14 below 1/4);
//   * operands are pre-expanded once per call into MFMA fragment order ([tile][kstep][lane] x 16 B), so a wave fetches a
//     train tile's fragment with KS perfectly coalesced 1 KiB loads straight from L2 (the expanded train set of a C2
//     image is 1 MiB) -- no LDS, no barriers; the query fragments stay in registers for the whole kernel.
// Output: the same [batch][split][nq] uint2 table of packed (dist << dshift | local row) keys the VALU kernels write,
// merged by knn_hamming_merge_kernel.

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "mlpl_internal.h"


namespace mlpl {

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr float kEps = 1.0f / 16384.0f;  // 2^-14: row weight in the accumulator
// Rows of one split.  A candidate's value is I - (row - frame) * 2^-14 with I = nbits - 2 d an integer of magnitude <= 512 and the frame the
// first row of the tile being folded, so over a split of R rows the fraction lies in (-32 eps, R eps): R <= 8192 keeps it inside
// (-1/2, 1/2) -- rint() recovers I -- and a multiple of 2^-14 below 512 is exact in fp32.  (Up to round 4 the cap was 4096, which cut every
// 8192-row train set of a full batch in two although the chip was already full: partials, tickets and a fold for nothing.)
constexpr int kMaxRowsPerSplit = 8192;
// Accumulator bias of the in-kernel-expansion instances of the LDS-ring kernel (XP): their chains start at kAccBias - row * 2^-14 instead of
// -row * 2^-14, so a value is kAccBias + I - (row - frame) * 2^-14.  Around zero a random pair's I = 0 +- 16 flips the float's sign and moves
// its exponent from one register write to the next, which re-aligns the whole mantissa, the constant row fraction included; with the bias
// every typical value stays inside the binade [512, 1024): sign and exponent never change, the fraction keeps its 14 low mantissa bits and
// only the integer part's 7-9 bits move -- fewer bits switching per MFMA in a launch whose clock is power-limited.  Same
// instruction stream; the decode removes the bias before a key is formed, so every byte that leaves the kernel is what it was.
// Exactness: every value, final or partial sum of a chain, is kAccBias + I + f * 2^-14 with |I| <= 256 (KS = 4: 256 bits) and f in
// [-31, kMaxRowsPerSplit - 32]; it must be a multiple of 2^-14 of magnitude below 1024 (24-bit significand), and its fraction stays inside
// (-1/2, 1/2) as before, so rint() returns kAccBias + I.  tests/test_hamming_acc_bias_rule.py restates this over every (I, f).
constexpr float kAccBias = 704.0f;
static_assert(kAccBias == (float)(int)kAccBias, "the bias is an integer: rint() of a value is kAccBias + I");
static_assert(kAccBias + 256.0f + (float)(kMaxRowsPerSplit - 32) / 16384.0f < 1024.0f, "largest value (identical rows, last tile) below 2^10: 2^-14 is exact");
static_assert(kAccBias - 256.0f - 31.0f / 16384.0f > -1024.0f, "smallest value (complementary rows) above -2^10");
static_assert(kAccBias - 64.0f >= 512.0f && kAccBias + 64.0f < 1024.0f, "typical data (|I| <= 64) stay inside the binade [512, 1024)");
// The 16x16x128 instance carries the ABSOLUTE row of the split in C instead of re-basing its running pairs: a value, final or partial sum of a
// chain, is kAccBias + I - r * 2^-14 with |I| <= 256 and r in [0, kMaxRowsPerSplit - 1] -- magnitude below 2^10, fraction inside (-1/2, 0], so
// rint() returns kAccBias + I and the decode reads the row from the fraction with frame 0 (tests/test_hamming_shape16_fit_rule.py: every (I, r)).
static_assert(kAccBias + 256.0f < 1024.0f && kAccBias - 256.0f - (float)(kMaxRowsPerSplit - 1) / 16384.0f > -1024.0f, "absolute rows: magnitude below 2^10");
static_assert((float)(kMaxRowsPerSplit - 1) / 16384.0f < 0.5f, "absolute rows: the fraction stays inside (-1/2, 0]");
static_assert(kAccBias - 64.0f - (float)(kMaxRowsPerSplit - 1) / 16384.0f >= 512.0f, "absolute rows: typical data stay inside the binade [512, 1024)");

__device__ __forceinline__ float fmax_raw(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float fmed3_raw(float a, float b, float c) {
    float r;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// 8 bits -> 8 fp4 nibbles (bit i -> nibble i): 1 -> 0x2 (+1.0), 0 -> 0xA (-1.0)
__device__ __forceinline__ uint32_t expand_byte(uint32_t x) {
    uint32_t t = (x | (x << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return 0xAAAAAAAAu ^ (t << 3);
}

// The {0, +1} form of the STREAMED (train) operand (option hamming_train01): bit 1 -> 0x2 (+1.0), bit 0 -> 0x0 (+0.0).  With the query
// operand still +-1,  sum_k t_k q'_k = pop(t & q) - pop(t & ~q) = pop(q) - hamming(t, q):  for a fixed query (a lane's column) the
// accumulator still orders the train rows by distance, all values are exact integers in [-256, 256], and half of the A operand's nibbles
// are zero (fewer toggling multiplier inputs: the sustained matrix-core clock is data dependent).  The decode adds pop(q).
__device__ __forceinline__ uint32_t expand_byte01(uint32_t x) {
    uint32_t t = (x | (x << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return t << 1;
}
// one 32-bit word -> the 16 bytes of its fragment (byte j of the word -> dword j), in either encoding
__device__ __forceinline__ u32x4 expand_word(uint32_t v) {
    return u32x4{expand_byte(v & 255u), expand_byte((v >> 8) & 255u), expand_byte((v >> 16) & 255u), expand_byte(v >> 24)};
}
__device__ __forceinline__ u32x4 expand_word01(uint32_t v) {
    return u32x4{expand_byte01(v & 255u), expand_byte01((v >> 8) & 255u), expand_byte01((v >> 16) & 255u), expand_byte01(v >> 24)};
}

// The BIT-PLANE rule of the in-kernel expansion (option hamming_expand_inkernel): every output dword of a 16-byte fragment is one plane of ONE
// raw 32-bit word -- nibble j of plane p carries bit 4 j + p -- and a nibble is 0x2 | bit << 3, i.e. bit 0 -> +1.0, bit 1 -> -1.0.  One mask and
// one v_lshl_or_b32 per output dword against the ~9 operations of expand_byte.  Which bit goes to which K position is free as long as both
// operands follow the same rule, and so is the sign convention: both operands flip together and every product is unchanged.  The four dwords
// of a fragment carry the planes 0, 2, 1, 3 in this order: the thread that forms dwords 2 i and 2 i + 1 needs planes i and i + 2, which are planes
// 0 and 2 of the word shifted right by i (kernel below).
__device__ __forceinline__ uint32_t expand_plane(uint32_t x, int p) { return ((x & (0x11111111u << p)) << (3 - p)) | 0x22222222u; }
// the same for planes 0 and 2 in the two instructions named above (left to itself the compiler shifts first and takes three; `twos` =
// 0x22222222 in a scalar register)
__device__ __forceinline__ uint32_t expand_plane0(uint32_t x, uint32_t twos) {
    uint32_t r;
    asm("v_lshl_or_b32 %0, %1, 3, %2" : "=v"(r) : "v"(x & 0x11111111u), "s"(twos));
    return r;
}
__device__ __forceinline__ uint32_t expand_plane2(uint32_t x, uint32_t twos) {
    uint32_t r;
    asm("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(r) : "v"(x & 0x44444444u), "s"(twos));
    return r;
}

// Rows of `nw` 32-bit words (word rows as the VALU path uses them) -> fragment order.  Lane (r = l & 31, h = l >> 5) of
// K-step s holds word h * KS + s of row 32 * tile + r, i.e. each lane owns KS CONSECUTIVE words of its row (one 16-byte
// load at KS = 4, and the wave reads one contiguous KiB); which 32 bits go to which K position is free as long as both
// operands use the same rule, and they do -- this kernel expands both.  Rows >= n and words >= nw read as zero bits (the
// same in both operands, so they add nothing to a distance).  `tiles` covers the padded row count.
// One launch: blockIdx.z = 0 queries, 1 train rows; one thread per (tile, lane), KS x 16 bytes out.
struct ExpandArgs {
    const uint32_t *src;
    size_t src_batch_words;
    int n, tiles;
    uint4 *dst;
};

template <int KS>
__global__ __launch_bounds__(256) void hamming_expand_kernel(ExpandArgs qa, ExpandArgs ta, int nw, int *__restrict__ counters,
                                                             int counters_per_batch, int train01) {
    const ExpandArgs A = blockIdx.z ? ta : qa;
    const int b = blockIdx.y;
    if (counters && blockIdx.x == 0 && blockIdx.z == 0)  // chunk counters of the dynamic-split kernel that follows in the stream
        for (int i = threadIdx.x; i < counters_per_batch; i += 256) counters[(size_t)b * counters_per_batch + i] = 0;
    const int i = blockIdx.x * 256 + threadIdx.x;  // tile * 64 + lane
    if (i >= A.tiles * 64) return;
    const int l = i & 63, tile = i >> 6;
    const int row = tile * 32 + (l & 31);
    const int w0 = (l >> 5) * KS;
    uint32_t v[KS];
    const uint32_t *p = A.src + (size_t)b * A.src_batch_words + (size_t)row * nw + w0;
    if (row < A.n && nw == 2 * KS) {  // whole words, KS * 4-byte aligned (rows are nw words): one vector load
        if constexpr (KS == 4) {
            const uint4 x = *reinterpret_cast<const uint4 *>(p);
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        } else if constexpr (KS == 8) {
            const uint4 x = reinterpret_cast<const uint4 *>(p)[0], y = reinterpret_cast<const uint4 *>(p)[1];
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
        } else if constexpr (KS == 2) {
            const uint2 x = *reinterpret_cast<const uint2 *>(p);
            v[0] = x.x, v[1] = x.y;
        } else {
            v[0] = p[0];
        }
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) v[s] = (row < A.n && w0 + s < nw) ? p[s] : 0u;
    }
    uint4 *out = A.dst + ((size_t)b * A.tiles + tile) * KS * 64 + l;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        u32x4 o = expand_word(v[s]);
        if (train01) o = expand_word01(v[s]);  // (only ever set for the train operand of the static LDS-ring kernel, which expands its queries itself)
        __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(out + s * 64));
    }
}

// The same expansion of a TRAIN set of 32-byte descriptors with one thread per (tile, K-step, lane) instead of per (tile, lane): for ONE
// image pair hamming_expand_kernel<4> is 64 workgroups with 16 expansions per thread -- a quarter of the chip, one long thread each; this
// form is one 256-thread workgroup per tile (256 for 8192 rows).  Same bytes at the same addresses.  (Round 6, the latency shape.)
__global__ __launch_bounds__(256) void hamming_expand_fine_kernel(ExpandArgs A, int train01) {
    constexpr int KS = 4;
    const int b = blockIdx.y;
    const int tile = blockIdx.x;   // gridDim.x == A.tiles
    const int l = threadIdx.x & 63, st = threadIdx.x >> 6;
    const int row = tile * 32 + (l & 31);
    const int w = (l >> 5) * KS + st;
    const uint32_t v = row < A.n ? A.src[(size_t)b * A.src_batch_words + (size_t)row * (2 * KS) + w] : 0u;
    u32x4 o = expand_word(v);
    if (train01) o = expand_word01(v);
    __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(A.dst + ((size_t)b * A.tiles + tile) * KS * 64 + st * 64 + l));
}

// Round 5: the UNSCALED form.  v_mfma_scale_f32_32x32x64_f8f6f4 is a two-part instruction (a scale-load prefix + the MFMA) that reads two
// more registers; with unit scales it computes what v_mfma_f32_32x32x64_f8f6f4 computes without them.  The compiler selects the unscaled
// opcode when both scale operands are the constant 0 (its encoding of "no scales").  Rounds 1-4 issued the scaled form with E8M0 0x7F
// (2^0) in a register: 35 cycles per MFMA in the probes against the nominal 32.  MLPL_MFMA_SCALED=1 rebuilds the old form for the A/B.
#ifndef MLPL_MFMA_SCALED
#define MLPL_MFMA_SCALED 0
#endif
__device__ __forceinline__ v16f mfma_fp4(uint4 a, uint4 b, v16f c) {
    const v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const v8i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    // cbsz = blgp = 4: fp4 operands (4 registers each)
#if MLPL_MFMA_SCALED
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);  // E8M0 scale 0x7F = 2^0 for both
#else
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, 0, 0, 0);
#endif
}

// Running top-2 (m1 >= m2) of a lane over the 16 candidates of one accumulator tile.  Four candidates per step, 5 VALU ops: with
// T = {m1, a, b} the second largest of T + {m2} is max(med3(T), m2) because m2 <= m1; two such pairs share one max3 for m2 (values are
// distinct, or -inf).
__device__ __forceinline__ void top2_update4(float &m1, float &m2, float a0, float a1, float a2, float a3) {
    const float s0 = __builtin_amdgcn_fmed3f(m1, a0, a1);
    const float t0 = __builtin_fmaxf(__builtin_fmaxf(m1, a0), a1);
    const float s1 = __builtin_amdgcn_fmed3f(t0, a2, a3);
    m1 = __builtin_fmaxf(__builtin_fmaxf(t0, a2), a3);
    m2 = __builtin_fmaxf(__builtin_fmaxf(m2, s0), s1);
}

// The BLOCK form of the update (option hamming_block_top2, the in-kernel-expansion instances of the LDS-ring kernel): only the MAXIMUM of a
// fixed block of the lane's 16 candidates is folded into the running pair.  m1 is then still the exact maximum of every row the lane has
// seen, and m2 is at least the maximum of every block but the one that holds m1's row: a candidate missing from m2 can only be a
// non-maximal member of that one block, which the epilogue re-scores from the raw descriptors (block_rescan).
// A block = accumulator registers 4 j .. 4 j + 3 = an aligned group of four consecutive train rows: four times max(max3(..), a) and one
// top2_update4 over the four maxima (spelt out in its order, two maxima at a time), 13 VALU ops against 20.
__device__ __forceinline__ void top2_update_blocks4(float &m1, float &m2, const v16f &acc) {
    auto max4 = [&](int j) { return __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(acc[4 * j], acc[4 * j + 1]), acc[4 * j + 2]), acc[4 * j + 3]); };
    const float g0 = max4(0), g1 = max4(1);
    const float s0 = __builtin_amdgcn_fmed3f(m1, g0, g1);
    const float t0 = __builtin_fmaxf(__builtin_fmaxf(m1, g0), g1);
    const float g2 = max4(2), g3 = max4(3);
    const float s1 = __builtin_amdgcn_fmed3f(t0, g2, g3);
    m1 = __builtin_fmaxf(__builtin_fmaxf(t0, g2), g3);
    m2 = __builtin_fmaxf(__builtin_fmaxf(m2, s0), s1);
}

// the train tile's row that accumulator register `reg` holds in a lane of half h
__device__ __forceinline__ int acc_local_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
// C of the first MFMA of every tile: minus the local row of accumulator register `reg` in this lane, times eps
__device__ __forceinline__ v16f row_weights(int h) {
    v16f c;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) c[reg] = -(float)acc_local_row(reg, h) * kEps;
    return c;
}
// the same for a ragged tile whose first row is `tile_row0`: rows >= nt start at -inf and stay there
__device__ __forceinline__ v16f row_weights_ragged(int h, int tile_row0, int nt) {
    v16f c;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int lr = acc_local_row(reg, h);
        c[reg] = (tile_row0 + lr < nt) ? -(float)lr * kEps : -INFINITY;
    }
    return c;
}

// Epilogue of every kernel: a lane's running pair -> two packed (dist << dshift | local row) keys (decode_key; -inf = no candidate takes
// the key 0xFFFFFFFF at the call site), then the top-2 of the four keys of the two lane halves (top2_across_halves).
// How the integer part ip of a value becomes a distance:
struct DistRule {
    int nbits;    // +-1 train operand: d = (nbits - ip) >> 1, nbits = 64 KS
    int train01;  // != 0: the {0, +1} train operand instead, d = qpop - ip with qpop = pop(query)
    int qpop;
    __device__ __forceinline__ int operator()(int ip) const { return train01 ? qpop - ip : (nbits - ip) >> 1; }
};
// A value is v = ip + (frame - local_row) * eps with `frame` the first row, relative to the split, of the last tile folded; the fraction
// lies inside (-1/2, 1/2), so rint() recovers ip.
__device__ __forceinline__ uint32_t decode_key(float v, float frame, int dshift, DistRule dist) {
    const float ip = rintf(v);
    const int d = dist((int)ip);
    const int lrow = (int)(frame - (v - ip) * 16384.0f);
    return ((uint32_t)d << dshift) | (uint32_t)lrow;
}
// the same for a value of a chain that started at kAccBias: rint() returns kAccBias + ip; the fraction is read as above
__device__ __forceinline__ uint32_t decode_key_biased(float v, float frame, int dshift, DistRule dist) {
    const float ipb = rintf(v);
    const int d = dist((int)(ipb - kAccBias));
    const int lrow = (int)(frame - (v - ipb) * 16384.0f);
    return ((uint32_t)d << dshift) | (uint32_t)lrow;
}
// the two lane halves hold disjoint rows of the same query: top-2 of the four keys, in both halves
__device__ __forceinline__ uint2 top2_across_halves(const uint32_t (&k)[2]) {
    const uint32_t o0 = __shfl_xor(k[0], 32), o1 = __shfl_xor(k[1], 32);
    uint32_t k0 = k[0], k1 = k[1];
    k1 = umed3(k0, k1, o0);
    k0 = min(k0, o0);
    k1 = umed3(k0, k1, o1);
    k0 = min(k0, o1);
    return make_uint2(k0, k1);
}

// Epilogue of the block update (top2_update_blocks4): the exact second of a query.  After top2_across_halves k0 is the
// query's exact best key; the merged second can only be short of the non-maximal rows of the ONE block that holds the best row (the other
// lane half's m1 is the exact maximum of its rows).  Those rows are re-scored here from the raw descriptors -- xor + popcount over the eight
// words, the key (distance << dshift | local row) the decode forms -- and the smallest of them is returned (0xFFFFFFFF: none), in both lanes
// of the query, for the caller's min() with the merged second.  The block is the aligned group of four rows around the best, 128 contiguous
// bytes; the two lanes of the query (he = 0, 1) take two rows each.
// `q8` = the query's eight raw words; `rbase` = the first row of the split (local row 0), `rows` = the image pair's train rows from there on
// (>= 1).  The best row itself and rows >= `rows` (the ragged last tile) do not count; every address is clamped to the pair's last row, so
// nothing behind the train set is read, and k0 = 0xFFFFFFFF (no candidate at all) yields none.  Branch-free: every lane of the wave loads.
struct __attribute__((packed, aligned(4))) RawRow {   // (a train row is word-aligned, not more: the in-kernel expansion asks for no more)
    uint32_t w[8];
};
__device__ __forceinline__ uint32_t block_rescan(uint32_t k0, const uint32_t (&q8)[8], const char *rbase, int rows, int dshift, int he) {
    const uint32_t lmask = (1u << dshift) - 1u;
    const int best = (int)(k0 & lmask);
    uint32_t res = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (best & ~3) + 2 * he + i;
        const RawRow t = *reinterpret_cast<const RawRow *>(rbase + (size_t)min(r, rows - 1) * 32);
        int d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += __popc(t.w[j] ^ q8[j]);
        const uint32_t key = ((uint32_t)d << dshift) | (uint32_t)r;
        res = (r != best && r < rows && k0 != 0xFFFFFFFFu) ? min(res, key) : res;
    }
    return min(res, (uint32_t)__shfl_xor(res, 32));
}

// XCD-aware work assignment.  Workgroups go round-robin to the 8 XCDs (each with its own L2), so workgroup L runs on XCD L % 8.  The
// work items are ordered (batch item, split, query group or block) and XCD x takes the x-th contiguous eighth of that order: with 8
// image pairs per launch every XCD streams ONE pair's train fragments (1 MiB at C2) through its L2 instead of all eight; with one pair
// an XCD sees an eighth of the train splits.  Returns the workgroup's place in that order (the grid is padded to a multiple of 8).
__device__ __forceinline__ int xcd_block_item() {
    const int per_xcd = (int)(gridDim.x >> 3);
    return (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
}

// Diagnostics only ("hamming_stamps" option): shader-clock and 100 MHz real-time deltas per wave.
__device__ __forceinline__ void clock_start(bool on, unsigned long long &st_c, unsigned long long &st_r) {
    if (on) {
        st_c = __builtin_amdgcn_s_memtime();
        st_r = __builtin_amdgcn_s_memrealtime();
    }
}
// the wave's record: {cycles, ticks, tiles * qt units | hardware ids, start tick}
__device__ __forceinline__ void clock_stamp(unsigned long long *o, unsigned long long st_c, unsigned long long st_r, int tiles, int qt) {
    o[0] = __builtin_amdgcn_s_memtime() - st_c;
    o[1] = __builtin_amdgcn_s_memrealtime() - st_r;
    // HW_REG_HW_ID (4): wave/simd/cu/sh/se ids; HW_REG_XCC_ID (20): the XCD
    const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));
    o[2] = (unsigned long long)tiles * qt | ((unsigned long long)(hw & 0xFFFFFu) << 32) | ((unsigned long long)(xcc & 15u) << 56);
    o[3] = st_r;
}

// One 4 KiB tile of an LDS ring (four K-steps, 1 KiB apart) into registers; `addr` = the lane's LDS byte address of K-step 0.
// The tile is read back with hand-written ds_read_b128: for a compiler-visible LDS load the waitcnt pass would first drain EVERY
// outstanding LDS-DMA (vmcnt(0): it cannot know that the copies in flight target other ring slots), which serialises the prefetch.
// The reads return in order, so K-step s is complete once at most 3 - s of them are outstanding.
__device__ __forceinline__ void ring_read_tile(u32x4 (&r)[4], uint32_t addr) {
    asm volatile(
        "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072"
        : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
        : "v"(addr)
        : "memory");
    asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[0]));
    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[1]));
    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[2]));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[3]));
}

// KS K-steps of 64 bits, QT query tiles (32 queries each) per wave.  A wave's work item is (batch item, train split, query
// group of QT tiles); the 4 waves of a workgroup are independent (no LDS, no barriers) and take consecutive items, i.e.
// neighbouring query groups of the same train split, so they stream the same train fragments through the CU's L1.
template <int KS, int QT>
__global__ __launch_bounds__(256, (KS >= 8 ? 2 : 3)) void knn_hamming_mfma_kernel(
    const uint4 *__restrict__ qfrag, size_t q_batch_u4, const uint4 *__restrict__ tfrag, size_t t_batch_u4, int nq, int nt,
    int rows_per_split, int nsplit, int dshift, int qgroups, int n_items, uint2 *__restrict__ part,
    unsigned long long *__restrict__ stamps) {
    const int l = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    unsigned long long st_c = 0, st_r = 0;
    clock_start(stamps != nullptr, st_c, st_r);
    // xcd_block_item() at wave granularity: item = (batch item, train split, query group).  Spelt out: through the helper the <2, 4> instance
    // comes out with a differently associated address shift (same work, another instruction stream).
    const int per_xcd = (int)(gridDim.x >> 3);
    const int item = ((int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3)) * 4 + w;
    if (item >= n_items) return;  // wave-uniform; the kernel has no barriers
    const int qg = item % qgroups;
    const int split = (item / qgroups) % nsplit;
    const int b = item / (qgroups * nsplit);
    const int qt0 = qg * QT;  // first query tile of this wave (the fragment buffer is padded to whole groups)
    const uint4 *qf = qfrag + (size_t)b * q_batch_u4 + (size_t)qt0 * KS * 64 + l;
    const uint4 *tf = tfrag + (size_t)b * t_batch_u4 + l;

    uint4 bq[QT][KS];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s) bq[t][s] = qf[(size_t)(t * KS + s) * 64];

    const int h = l >> 5;
    const v16f cinit = row_weights(h);

    const int row0 = split * rows_per_split;
    const int row1 = min(nt, row0 + rows_per_split);
    const int tile0 = row0 >> 5;
    const int ntiles = (row1 - row0 + 31) >> 5;  // >= 1: the host never launches an empty split

    float m1[QT], m2[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) m1[t] = m2[t] = -INFINITY;

    // fragment stream of this split; the buffer carries one spare tile, so the prefetch past the last tile needs no clamp
    const uint4 *tp = tf + (size_t)tile0 * KS * 64;
    uint4 fa[KS], fb[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) fa[s] = tp[s * 64];

    // one train tile against the wave's QT query tiles: KS MFMAs + 22 VALU ops per query tile
    auto tile_body = [&](const uint4 (&a)[KS], const v16f &c0) {
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            v16f acc = mfma_fp4(a[0], bq[t][0], c0);
#pragma unroll
            for (int s = 1; s < KS; ++s) acc = mfma_fp4(a[s], bq[t][s], acc);
            // re-base the running pair to this tile's row origin (exact; -inf stays -inf)
            m1[t] += 32.0f * kEps;
            m2[t] += 32.0f * kEps;
#pragma unroll
            for (int reg = 0; reg < 16; reg += 4) top2_update4(m1[t], m2[t], acc[reg], acc[reg + 1], acc[reg + 2], acc[reg + 3]);
        }
    };

    // only the last tile of the train set can be ragged; it gets its own C (rows >= nt start at -inf and stay there)
    const bool ragged = row0 + ntiles * 32 > nt;
    const int nfull = ragged ? ntiles - 1 : ntiles;
    int it = 0;
    for (; it + 2 <= nfull; it += 2) {  // ping-pong between the two fragment sets: no register copies in the steady state
#pragma unroll
        for (int s = 0; s < KS; ++s) fb[s] = tp[(KS + s) * 64];
        tile_body(fa, cinit);
        tp += 2 * KS * 64;
#pragma unroll
        for (int s = 0; s < KS; ++s) fa[s] = tp[s * 64];
        tile_body(fb, cinit);
    }
    if (it < nfull) {
#pragma unroll
        for (int s = 0; s < KS; ++s) fb[s] = tp[(KS + s) * 64];
        tile_body(fa, cinit);
#pragma unroll
        for (int s = 0; s < KS; ++s) fa[s] = fb[s];
    }
    if (ragged) {
        tile_body(fa, row_weights_ragged(h, row0 + nfull * 32, nt));
    }

    // decode (frame = last tile): v = (64 KS - 2 d) + (32 (ntiles - 1) - local_row) * eps
    const float frame = (float)(32 * (ntiles - 1));
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        uint32_t k[2];
        const float mm[2] = {m1[t], m2[t]};
#pragma unroll
        for (int j = 0; j < 2; ++j)  // (-inf: no candidate)
            k[j] = mm[j] == -INFINITY ? 0xFFFFFFFFu : decode_key(mm[j], frame, dshift, DistRule{64 * KS, 0, 0});
        const uint2 kk = top2_across_halves(k);
        const int q = (qt0 + t) * 32 + (l & 31);
        if (h == 0 && q < nq) part[((size_t)b * nsplit + split) * nq + q] = kk;
    }
    if (stamps && l == 0) clock_stamp(stamps + (size_t)item * 4, st_c, st_r, ntiles, QT);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// KS = 4 (descriptors of 17..32 bytes: ORB-256) with the train tiles SHARED by the 4 waves of a workgroup through an LDS ring.
// Why (tools/hamming_unit_probe3.hip, in-kernel clock stamps): a 1 KiB global_load_dwordx4 occupies the CU's one vector-memory/L1 path
// (64 B/clk) for 16 cycles; with every wave fetching its own 4 KiB per tile the four SIMDs of a CU need 64 of the ~130 cycles a unit
// costs them, and the fragment double buffer (32 VGPRs) holds the kernel at 3 waves per SIMD, where a wave's ~44-cycle MFMA issue
// interval is not hidden (178-193 cycles per unit per SIMD measured; MFMA and VALU do not overlap on a SIMD, they add: ~90 + ~40).
// Here wave w copies K-step w of every tile straight into LDS (global_load_lds_dwordx4: no staging registers, a quarter of the L1
// traffic), all four read the tile back with ds_read_b128 (LDS: 256 B/clk), and 120 VGPRs give 4 waves per SIMD.
// Ring protocol (NB = 4 slots of 4 KiB, prefetch distance D = 2, one s_barrier per tile): in iteration `it` a wave issues the copy of
// tile it + 2, waits for its own piece of tile `it` (vmcnt counts LDS-DMA in issue order), and the barrier makes all four pieces
// visible.  Slot (it + 2) % 4 was last read in iteration it - 2, and a wave that has passed the barrier of iteration it - 1 knows that
// every wave has finished iteration it - 2 (its MFMAs consumed those reads), so the copy cannot overtake a reader.
// ---------------------------------------------------------------------------------------------------------------------------------
// Fused epilogue (`fuse.idx` != nullptr; QT = 2 or 4): the merge of the splits, the ratio predicate and the per-64-query pass counts -- the
// work of knn_hamming_merge_kernel -- happen HERE.  One split: straight from the registers that hold the final top-2 (no partial table at
// all).  Several splits: every workgroup writes its partial top-2 as before, then takes a ticket of its (image pair, query block); the
// workgroup that draws the last ticket folds the splits' partials of its 128 * QT queries (64-bit (distance, global row) keys, as the
// merge kernel) and resets the ticket counter.  Same outputs as the two-kernel path bit for bit (min over keys is order-independent).
struct HammingFuse {
    int32_t *idx, *dist, *group_counts;
    int *tickets;   // [batch][qblocks], zero before the launch; left zero by the last workgroup
    int k;
    float ratio;
    int train01;    // the train fragments are {0, +1} (hamming_expand_kernel train01): accumulator = pop(query) - distance
    // Clock record of this launch (option hamming_stamps = 2; nullptr otherwise): thread 0 of work item 0 leaves {shader-clock cycles,
    // 100 MHz ticks, start tick, launch number} of its workgroup's lifetime -- one 32-byte store per launch, the cost of the facility.
    unsigned long long *clk;
    unsigned long long launch_no;
};

// NW (round 5) = waves per workgroup, 4 or 8: waves 0..3 copy one K-step of every tile each, ALL NW read it -- with 8 waves a tile is
// fetched and a barrier passed once per eight units' worth of query tiles instead of four (tools/hamming_unit_probe3.hip `ringnw`: 167.9 ->
// 159.1 cycles per unit per SIMD).  A workgroup then serves NW * QT query tiles of one (image pair, train split).
// PD (round 5) = prefetch distance in tiles (2, 4 or 6): the copy of tile it + PD is issued in iteration it; the ring has NB >= PD + 2 slots.
//
// XP (option hamming_expand_inkernel, NW = 8 and PD = 2 only) = the workgroup expands the train tiles it consumes ITSELF: `tsrc` is the raw
// train set (rows of 8 words, `t_batch` words per image pair) instead of the fragment buffer, hamming_expand_kernel does not run and the
// 4x expanded copy of the train set is neither written to memory nor read back.
//   * Raw ring, NR = 4 slots of 1 KiB, raw tile t in slot (t + 3) & 3: waves 0..3 copy a quarter each of the raw tile (32 rows x 8 words,
//     contiguous in memory) with 4-byte LDS-DMA, a scalar base plus a 32-bit lane offset that is clamped to the last word of the image pair's
//     train set (the rows of a ragged last tile behind it start at -inf through its C and never count; nothing past the pair's rows is read).
//   * Fragment ring, 2 slots of 4 KiB in the fragment order the tile body reads: lane (r, h) of K-step s holds the four planes of raw word
//     4 h + s of row r.  Wave w expands word w of all 32 rows: lane l reads the word of row l >> 1 and writes dwords 2 (l & 1), 2 (l & 1) + 1,
//     so a wave writes 512 CONTIGUOUS bytes with ds_write_b64 (no bank conflict; the read is a 4-way conflict of one ds_read_b32).
//   * Protocol, one s_barrier per tile plus one in the prologue: in iteration `it` a copying wave issues the copy of raw tile it + 2 and waits
//     for its own piece of raw tile it + 1 (vmcnt(1)); behind the barrier every wave reads its word of raw tile it + 1 together with the
//     fragments of tile `it`, expands it into fragment slot (it + 1) & 1 and runs the body of tile `it`.  The prologue does the same for tile 0.
//     Slot reuse: a wave past the barrier of iteration `it` knows that every wave has finished the body of it - 1 (its MFMAs consumed those
//     reads), so fragment slot (it + 1) & 1 is free, and that every wave's writes of tile `it` have completed (lgkmcnt(0) before the barrier).
//     The raw slot of tile it + 2 last held tile it - 2, read behind the barrier of iteration it - 3 and complete before that of it - 2; the copy
//     is issued behind the barrier of it - 1.  The tile after the last one does not exist: the last iteration expands a stale raw slot into the
//     free fragment slot, which nobody reads -- cheaper than a branch around the hand-scheduled LDS sequence.
//   * Unrolled form (the production instance, ST = false): while a PAIR of tiles it = 2 p, 2 p + 1 with both its copies (tiles it + 2, it + 3) lies
//     inside the split's full tiles, the pair runs as straight-line code -- per tile still: the copy of tile it + 2, vmcnt(1) lgkmcnt(0), one
//     s_barrier, the raw word of tile it + 1 and the fragments of tile `it` read, fragment slot (it + 1) & 1 written, the body.  It is the
//     protocol above iteration by iteration, so the slot-reuse argument holds word for word; only the addresses are formed differently: the
//     fragment slots are it & 1 = J and (it + 1) & 1, the raw slot read is (it + 4) & 3 = 2 (p & 1) + J, so everything but 2 (p & 1) is a
//     constant in an instruction's offset field, and the lane parts are formed once in front of the loop.  The first KS waves and the others
//     run their own copy of the loop (no test of the role per tile).  The rolled loop takes what is left (at most three full tiles) with the
//     vmcnt(0) waits of the last two iterations, the clamp of the copy -- which can bind in the last tile only, never inside a pair -- and the
//     stale-slot expansion; the ragged tile follows as before.
//   * ST (option hamming_stamps = 1) = the instance with the per-tile clock stamp; it keeps the rolled loop throughout.
//   * BT (option hamming_block_top2; 0 or 4, non-zero with XP only: the epilogue needs the raw train rows) = the running top-2 folds the maxima
//     of blocks of four candidates instead of the candidates (top2_update_blocks4: 13 VALU ops per unit against 20) and the epilogue re-scores the
//     best row's block (block_rescan) before any store, so the partials of a split are its exact top-2 and everything behind them is unchanged.
template <int QT, int PRIO, int NW = 4, int PD = 2, bool XP = false, bool ST = false, int BT = 0>
__global__ __launch_bounds__(64 * NW, 4) void knn_hamming_mfma_lds_kernel(
    const uint32_t *__restrict__ qw, size_t q_batch_words, const void *__restrict__ tsrc, size_t t_batch, int nq, int nt,
    int rows_per_split, int nsplit, int dshift, int qblocks, int n_items, uint2 *__restrict__ part,
    unsigned long long *__restrict__ stamps, const int32_t *__restrict__ split_tile0, HammingFuse fuse) {
    constexpr int KS = 4, NB = XP ? 2 : PD == 2 ? 4 : 8, NR = 4;
    static_assert(PD == 2 || PD == 4 || PD == 6, "prefetch distance");
    static_assert(!XP || (NW == 8 && PD == 2), "the in-kernel expansion exists for eight waves and a prefetch distance of 2");
    static_assert(BT == 0 || (XP && PRIO == 0 && BT == 4), "the block update needs the raw train rows of the in-kernel expansion");
    __shared__ __attribute__((aligned(16))) uint4 ring[NB][KS * 64];
    __shared__ __attribute__((aligned(16))) uint32_t raw_ring[XP ? NR * 256 : 1];   // (unused, hence not allocated, without XP)
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long st_c = 0, st_r = 0;
    clock_start(stamps || fuse.clk, st_c, st_r);
    const int item = xcd_block_item();  // (workgroup granularity: item = (batch item, train split, block of NW query groups))
    if (item >= n_items) return;  // workgroup-uniform: no wave of this workgroup reaches a barrier
    const int qb = item % qblocks;
    const int split = (item / qblocks) % nsplit;
    const int b = item / (qblocks * nsplit);
    const int qt0 = (qb * NW + w) * QT;
    const int h = l >> 5;

    uint4 bq[QT][KS];   // the wave's query fragments (filled below, behind the first tile copies)
    // (row_weights(h) spelt out: through the helper the scalar prologue of twelve of the fourteen instances comes out in another order)
    // (XP: every chain starts at kAccBias, see the constant)
    v16f cinit;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        if constexpr (XP) cinit[reg] = kAccBias - (float)acc_local_row(reg, h) * kEps;
        else cinit[reg] = -(float)acc_local_row(reg, h) * kEps;
    }

    // split geometry: equal splits, or the age-aware table of the launcher (tiles [tab[s], tab[s + 1]) per image pair)
    int row0 = split * rows_per_split;
    int row1 = min(nt, row0 + rows_per_split);
    if (split_tile0) {
        row0 = 32 * split_tile0[(size_t)b * (nsplit + 1) + split];
        row1 = min(nt, 32 * split_tile0[(size_t)b * (nsplit + 1) + split + 1]);
    }
    const int tile0 = row0 >> 5;
    const int ntiles = (row1 - row0 + 31) >> 5;

    float m1[QT], m2[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) m1[t] = m2[t] = -INFINITY;

    // my piece (K-step w) of the split's first tile; a tile is KS * 64 uint4 = 4 KiB, contiguous
    // (XP: my quarter of the raw tile instead; a raw tile is 32 rows x 8 words = 1 KiB, contiguous)
    const uint4 *tbase = (const uint4 *)tsrc + (size_t)b * t_batch + (size_t)tile0 * KS * 64 + (size_t)w * 64;  // wave-uniform
    const char *rbase = (const char *)tsrc + ((size_t)b * t_batch + (size_t)tile0 * 32 * (2 * KS)) * 4;         // wave-uniform
    const uint32_t raw_last = (uint32_t)(nt - row0) * (8u * KS) - 4u;   // byte offset of the pair's last train word behind rbase
    // XP: the lane parts of every address of the tile loop are formed ONCE (below, behind copies the compiler cannot see through: it would
    // re-form them from the lane index per tile, or keep the lane index alive beside them -- 128 registers are all in use): where the lane reads
    // the fragments (xp_frag), its raw word (xp_raw), where it writes its two planes (xp_plane), the plane shift l & 1 (xp_sh), and the byte
    // offset behind rbase of its word of raw tile xp_it0 + PD (xp_voff; the unrolled loop advances both by two tiles at a time).
    uint32_t xp_frag = 0, xp_raw = 0, xp_plane = 0, xp_sh = 0, xp_voff = 0;
    int xp_it0 = 0;
    auto copy_tile = [&](int t_rel) {
        if (NW > KS && w >= KS) return;  // (wave-uniform: the K-steps are copied by the first KS waves)
        if constexpr (XP) {
            const uint32_t off = min(xp_voff + (uint32_t)(t_rel - PD - xp_it0) * 1024u, raw_last);
            __builtin_amdgcn_global_load_lds((const void *)(rbase + off),
                                             (__attribute__((address_space(3))) void *)&raw_ring[((t_rel + NR - 1) & (NR - 1)) * 256 + w * 64], 4, 0, 0);
        } else {
            __builtin_amdgcn_global_load_lds((const void *)(tbase + (size_t)t_rel * KS * 64 + l),
                                             (__attribute__((address_space(3))) void *)&ring[t_rel & (NB - 1)][w * 64], 16, 0, 0);
        }
    };
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0] + (uint32_t)l * 16u;
    const uint32_t raw_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&raw_ring[0];
    const uint32_t frag_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0];
    // XP: where this lane reads its raw word of tile `t_rel` and where it writes the two planes it forms (see the protocol above)
    if constexpr (XP) {
        const uint32_t lx = (uint32_t)l;
        xp_frag = ring_lds;
        xp_raw = raw_lds + (uint32_t)w * 4u + (lx >> 1) * 32u;
        xp_plane = frag_lds + (uint32_t)(w & 3) * 1024u + (uint32_t)(w >> 2) * 512u + lx * 8u;
        xp_sh = lx & 1u;
        xp_voff = PD * 1024u + (uint32_t)w * 256u + lx * 4u;
        asm volatile("" : "+v"(xp_frag), "+v"(xp_raw), "+v"(xp_plane), "+v"(xp_sh), "+v"(xp_voff));
    }
    auto raw_addr = [&](int t_rel) { return xp_raw + (uint32_t)((t_rel + NR - 1) & (NR - 1)) * 1024u; };   // (raw tile t in slot (t + 3) & 3)
    auto plane_addr = [&](int t_rel) { return xp_plane + (uint32_t)(t_rel & 1) * (KS * 1024u); };
    auto expand_pair = [&](uint32_t x) {
        const uint32_t y = x >> xp_sh;   // dwords 0, 1 = planes 0, 2; dwords 2, 3 = planes 1, 3
        return u32x2{expand_plane0(y, 0x22222222u), expand_plane2(y, 0x22222222u)};
    };
    // the arithmetic of one tile: r[] = the tile's four K-steps in fragment order
    auto tile_math = [&](const u32x4 (&r)[KS], const v16f &c0) {
        uint4 a[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = make_uint4(r[s].x, r[s].y, r[s].z, r[s].w);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            v16f acc = mfma_fp4(a[0], bq[t][0], c0);
#pragma unroll
            for (int s = 1; s < KS; ++s) acc = mfma_fp4(a[s], bq[t][s], acc);
            m1[t] += 32.0f * kEps;
            m2[t] += 32.0f * kEps;
            if constexpr (BT == 4) {
                top2_update_blocks4(m1[t], m2[t], acc);
                // (one accumulator tile alive at a time, as in the dynamic kernel below: without this tie the instance takes 128 registers and
                // 16 bytes of scratch around the loops; with it 126 and none, in the same order of MFMAs and updates)
                asm volatile("" : "+v"(m1[t]), "+v"(m2[t]), "+v"(a[0].x));
                continue;
            }
#pragma unroll
            for (int reg = 0; reg < 16; reg += 4) {
                if constexpr (PRIO == 3) {
                    // Experiment (round 6; option hamming_mfma_prio = 3): wave-uniform skip.  A group of four rows changes a lane's
                    // running pair only if its largest value beats the lane's m2; after the first eighth of a split fewer than half of the
                    // groups do so in ANY lane.  3 ops (max3, max, compare) + a scalar branch instead of the 5-op update when none does.
                    // MEASURED NEGATIVE (gpurun_out/r6/hamming_skip_ab*.log, profiles/README.md): same outputs, the shader clock RISES from
                    // 1.84-1.97 to 2.06-2.17 GHz (less switching per cycle: the launch is power-limited), yet the kernel takes 0.376-0.383 ms
                    // against 0.363-0.379 -- the four VCC round trips per unit cost more cycles than the skipped updates save.  Off.
                    const float g = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(acc[reg], acc[reg + 1]), acc[reg + 2]), acc[reg + 3]);
                    if (__builtin_amdgcn_ballot_w64(g > m2[t]) == 0) continue;
                }
                top2_update4(m1[t], m2[t], acc[reg], acc[reg + 1], acc[reg + 2], acc[reg + 3]);
            }
        }
    };
    auto tile_body = [&](int it, const v16f &c0) {
        u32x4 r[KS];
        const uint32_t addr = (XP ? xp_frag : ring_lds) + (uint32_t)(it & (NB - 1)) * (KS * 1024u);
        if constexpr (XP) {
            uint32_t x;
            const uint32_t ra = raw_addr(it + 1), wa = plane_addr(it + 1);
            asm volatile(
                "ds_read_b32 %4, %6\n\tds_read_b128 %0, %5\n\tds_read_b128 %1, %5 offset:1024\n\tds_read_b128 %2, %5 offset:2048\n\t"
                "ds_read_b128 %3, %5 offset:3072"
                : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(x)
                : "v"(addr), "v"(ra)
                : "memory");
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x));
            const u32x2 o = expand_pair(x);
            asm volatile("ds_write_b64 %0, %1" ::"v"(wa), "v"(o) : "memory");
            // (in order behind the four fragment reads: K-step s is complete once at most 4 - s operations are outstanding)
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(r[0]));
            asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[1]));
            asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[2]));
            asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[3]));
        } else {
            ring_read_tile(r, addr);
        }
        tile_math(r, c0);
    };

#pragma unroll
    for (int t = 0; t < PD; ++t)
        if (t < ntiles) copy_tile(t);
    // (round 5: the first two tile copies are in flight BEFORE the query rows are fetched and expanded -- the two global latencies of a
    // workgroup's prologue overlap instead of adding; vmcnt retires in issue order, so the query loads' own wait also covers these copies,
    // which the first arrive() would wait for anyway)
    // The query operand is expanded to fp4 HERE, once per wave, from the raw 32-byte descriptors (lane (r, h) owns words 4h..4h+3 of its
    // row: one 16-byte load per tile; the same word -> K-position rule as hamming_expand_kernel, which now runs for the train set only --
    // that one has to exist in fragment order in memory because it is streamed into LDS by DMA).  Rows >= nq read as zero bits.
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int row = (qt0 + t) * 32 + (l & 31);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row < nq) v = *reinterpret_cast<const uint4 *>(qw + (size_t)b * q_batch_words + (size_t)row * (2 * KS) + (size_t)h * KS);
        const uint32_t vs[KS] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if constexpr (XP)   // (the rule of the train operand)
                bq[t][s] = make_uint4(expand_plane(vs[s], 0), expand_plane(vs[s], 2), expand_plane(vs[s], 1), expand_plane(vs[s], 3));
            else {
                const u32x4 o = expand_word(vs[s]);
                bq[t][s] = make_uint4(o.x, o.y, o.z, o.w);
            }
    }
    if constexpr (XP) {
        // tile 0: the query loads' wait has covered the first copies (see above); one barrier makes the four quarters visible, then every
        // wave expands its word of the tile into fragment slot 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        uint32_t x;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(x) : "v"(raw_addr(0)) : "memory");
        const u32x2 o = expand_pair(x);
        asm volatile("ds_write_b64 %0, %1" ::"v"(plane_addr(0)), "v"(o) : "memory");
    }

    // only the last tile of the train set can be ragged; it runs after the loop with its own C (rows >= nt start at -inf and stay there)
    const bool ragged = row0 + ntiles * 32 > nt;
    const int nfull = ragged ? ntiles - 1 : ntiles;
    // own piece of tile `it` landed <=> at most the copies of the tiles after it are still in flight (LDS-DMA retires in issue order)
    // (slot (it + PD) % NB was last read in iteration it + PD - NB <= it - 2, and a wave that has passed the barrier of iteration it - 1 knows
    // that every wave has finished iteration it - 2)
    auto arrive = [&](int it) {
        if constexpr (XP) {
            // own quarter of raw tile it + 1 landed; own planes of tile `it` (written in the previous iteration, or the prologue) complete
            if (it + PD < ntiles) {
                copy_tile(it + PD);
                asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            return;
        }
        if (it + PD < ntiles) {
            copy_tile(it + PD);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PD) : "memory");
        } else {
            const int ahead = ntiles - 1 - it;  // copies still allowed in flight: those of the tiles behind this one (< PD)
            if (PD > 4 && ahead == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else if (PD > 4 && ahead == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (PD > 2 && ahead == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else if (PD > 2 && ahead == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else if (ahead == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    };
    // Optional (PRIO, off by default): the hardware arbitrates oldest-first among equal priorities, so with identical work items the four
    // resident waves of a SIMD finish one after the other (28 -> 50 us measured).  Rotating s_setprio on a clock slice (2048 shader
    // cycles ~ 1 us) by (time + wave slot) makes them finish together (38 -> 50 us) -- but the launch is no shorter: the SIMD's
    // throughput is the same either way.  Kept as a measured negative result and a diagnostic.  (Round 5, eight-wave workgroups, one split per
    // 8192-row train set, i.e. exactly two workgroups resident per CU for the whole launch: unrotated the older workgroup finishes at 468k
    // cycles and the younger at 697k; rotated both finish at ~740k -- 6 % MORE cycles.  Strict oldest-first is the better schedule.
    // Priority by a workgroup's OWN progress instead -- high and low alternating every 16 / 32 / 64 tiles, one s_setprio per segment, no clock
    // read -- lets the younger workgroup catch up at every boundary: the older one then finishes at 288-306 us instead of 247 and the launch
    // takes 375.2-376.6 us against 375.7 (gpurun_out/r5/prio_progress_ab.log).  So the half-occupied last third is NOT slower per unit: the
    // SIMD delivers the same units per cycle with two resident waves as with four, and the staggered finish costs nothing.)
    const int wslot = (int)(__builtin_amdgcn_s_getreg(4 | (0 << 6) | (3 << 11)) & 3u);  // HW_ID.wave_id: slot within the SIMD
    auto rotate_prio = [&]() {
        if (PRIO != 1) return;
        const int p = (int)(((unsigned)(__builtin_amdgcn_s_memtime() >> 11) + (unsigned)wslot) & 3u);
        if (p == 0) __builtin_amdgcn_s_setprio(0);
        else if (p == 1) __builtin_amdgcn_s_setprio(1);
        else if (p == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
    };
    int it = 0;
    if constexpr (XP && !ST) {
        // Steady state, unrolled by the period of the fragment ring: pairs of tiles it = 2 p + J.  The fragment slots and, thanks to the rotated
        // raw slots (tile t in slot (t + 3) & 3: the pair reads raw slots 2 (p & 1) + J), the raw slot's low bit are constants of J and sit in the
        // offset fields of the LDS instructions; the raw slot's high bit is one add to xp_raw per PAIR.  A pair runs only while it + 3 < nfull,
        // so both tiles are full, have their copy of tile it + PD to issue (always vmcnt(1)) and copy a FULL tile: the clamp to raw_last
        // cannot bind and is left to the rolled tail below, which also takes an odd tile, the last PD tiles and the stale-slot expansion of
        // the last iteration.  (The ring period is four tiles; four tile bodies in one loop do not register-allocate in 128 VGPRs -- 276
        // bytes of scratch per lane -- and two do.)
        const uint32_t dma_lds = raw_lds + (uint32_t)w * 256u;
        int raw_step = 2 * 1024;   // +2 KiB, -2 KiB, ...: the raw slots 0, 1 <-> 2, 3 (scalar)
        auto tile_fixed = [&](auto jc, auto copier) {
            constexpr int J = decltype(jc)::value;
            __builtin_amdgcn_sched_barrier(0);   // (a tile's instructions stay inside the tile, as the back edge of the rolled loop keeps them)
            if constexpr (decltype(copier)::value) {
                // raw tile it + J + PD; the instruction's immediate offset J KiB applies to the source AND to the LDS destination, hence M0 =
                // the tile's slot minus J KiB (scalar arithmetic; xp_voff is the lane's offset of raw tile it + PD)
                const uint32_t m0 = dma_lds + (uint32_t)((it + J + PD + NR - 1) & (NR - 1)) * 1024u - (uint32_t)J * 1024u;
                __builtin_amdgcn_global_load_lds((const void *)(rbase + xp_voff), (__attribute__((address_space(3))) void *)(uintptr_t)m0, 4, J * 1024, 0);
            }
            asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            u32x4 r[KS];
            uint32_t x;
            asm volatile(
                "ds_read_b32 %4, %6 offset:%7\n\tds_read_b128 %0, %5 offset:%8\n\tds_read_b128 %1, %5 offset:%8+1024\n\t"
                "ds_read_b128 %2, %5 offset:%8+2048\n\tds_read_b128 %3, %5 offset:%8+3072"
                : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(x)
                : "v"(xp_frag), "v"(xp_raw), "i"(J * 1024), "i"((J & 1) * (KS * 1024))
                : "memory");
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x));
            const u32x2 o = expand_pair(x);
            asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(xp_plane), "v"(o), "i"(((J + 1) & 1) * (KS * 1024)) : "memory");
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(r[0]));
            asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[1]));
            asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[2]));
            asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[3]));
            tile_math(r, cinit);
        };
        // one copy of the loop per role: the first KS waves copy, the others only consume -- no test of the role inside the loop
        auto run_pairs = [&](auto copier) {
            while (it + 3 < nfull) {
                tile_fixed(std::integral_constant<int, 0>{}, copier);
                tile_fixed(std::integral_constant<int, 1>{}, copier);
                if constexpr (decltype(copier)::value) xp_voff += 2 * 1024, xp_it0 += 2;
                xp_raw += (uint32_t)raw_step;
                raw_step = -raw_step;
                it += 2;
            }
        };
        if (w < KS) run_pairs(std::true_type{});
        else run_pairs(std::false_type{});
        if (raw_step < 0) xp_raw -= 2 * 1024;   // (back to raw slot 0 for the rolled tail)
    }
    for (; it < nfull; ++it) {
        rotate_prio();
        arrive(it);
        if constexpr (!XP || ST)   // (the per-tile clock trace of hamming_stamps = 1; the in-kernel expansion has an instance of its own for it)
            if (stamps && l == 0 && it < 48) stamps[(size_t)n_items * NW * 4 + ((size_t)item * NW + w) * 48 + it] = __builtin_amdgcn_s_memtime();
        tile_body(it, cinit);
    }
    // XP: what follows the tile loop forms the lane and thread indices anew (lane count below this lane, wave number from its scalar register):
    // the loop does not use them any more, and kept alive across it for the ragged tile and the epilogue they would be spills
    int l_end = l, h_end = h;
    unsigned tid_end = threadIdx.x;
    if constexpr (XP) {
        l_end = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        h_end = l_end >> 5;
        tid_end = (unsigned)(w * 64 + l_end);
    }
    if (ragged) {
        arrive(nfull);
        if constexpr (XP) {   // (row_weights_ragged with the bias; rows >= nt still start at -inf and stay there)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int lr = acc_local_row(reg, h_end);
                cinit[reg] = (row0 + nfull * 32 + lr < nt) ? kAccBias - (float)lr * kEps : -INFINITY;
            }
        } else {
            cinit = row_weights_ragged(h_end, row0 + nfull * 32, nt);
        }
        tile_body(nfull, cinit);
    }

    // (the epilogue's addresses are formed from copies of the lane and tile indices the compiler cannot see through: formed in the prologue
    // they would have to live -- as spills: 128 registers are all in use -- across the main loop)
    int le = l_end, qt0e = qt0;
    asm volatile("" : "+v"(le), "+s"(qt0e));
    const int he = le >> 5;
    const float frame = (float)(32 * (ntiles - 1));
    int pass_acc = 0;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        // {0, +1} train operand (fuse.train01): the accumulator is pop(query) - distance.  The query's popcount is formed HERE, from the raw
        // words once more (both lane halves' shares of the row), so that the option costs the main loop no registers.
        int qpop = 0;
        if (fuse.train01) {
            const int row = (qt0e + t) * 32 + (le & 31);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < nq) v = *reinterpret_cast<const uint4 *>(qw + (size_t)b * q_batch_words + (size_t)row * (2 * KS) + (size_t)he * KS);
            const int pc = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
            qpop = pc + __shfl_xor(pc, 32);
        }
        uint32_t k[2];
        const float mm[2] = {m1[t], m2[t]};
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // (-inf: no candidate)
            const DistRule rule{64 * KS, fuse.train01, qpop};
            if constexpr (XP) k[j] = mm[j] == -INFINITY ? 0xFFFFFFFFu : decode_key_biased(mm[j], frame, dshift, rule);
            else k[j] = mm[j] == -INFINITY ? 0xFFFFFFFFu : decode_key(mm[j], frame, dshift, rule);
        }
        const uint2 kk = top2_across_halves(k);
        const int q = (qt0e + t) * 32 + (le & 31);
        const uint32_t k0 = kk.x;
        uint32_t k1 = kk.y;
        if constexpr (BT != 0) {
            if (fuse.k != 1) {   // (one neighbour: m1 is exact as it is)
                uint32_t q8[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                if (q < nq) {
                    const uint4 *qp = reinterpret_cast<const uint4 *>(qw + (size_t)b * q_batch_words + (size_t)q * (2 * KS));
                    const uint4 v0 = qp[0], v1 = qp[1];
                    q8[0] = v0.x, q8[1] = v0.y, q8[2] = v0.z, q8[3] = v0.w, q8[4] = v1.x, q8[5] = v1.y, q8[6] = v1.z, q8[7] = v1.w;
                }
                k1 = min(k1, block_rescan(k0, q8, rbase, nt - row0, dshift, he));
            }
        }
        if (fuse.idx && nsplit == 1) {  // the final top-2 of the query: outputs straight from the registers
            const uint32_t lmask = (1u << dshift) - 1u;
            bool pass = false;
            if (he == 0 && q < nq) {
                const size_t o = ((size_t)b * nq + q) * fuse.k;
                const int d0 = k0 == 0xFFFFFFFFu ? -1 : (int)(k0 >> dshift);
                fuse.idx[o] = k0 == 0xFFFFFFFFu ? -1 : (int)(row0 + (k0 & lmask));
                fuse.dist[o] = d0;
                if (fuse.k == 2) {
                    const int d1 = k1 == 0xFFFFFFFFu ? -1 : (int)(k1 >> dshift);
                    fuse.idx[o + 1] = k1 == 0xFFFFFFFFu ? -1 : (int)(row0 + (k1 & lmask));
                    fuse.dist[o + 1] = d1;
                    pass = (float)d0 < __fmul_rn(fuse.ratio, (float)d1);
                } else {
                    pass = true;
                }
            }
            const int c = __popcll(__ballot(pass));
            pass_acc = (t & 1) ? pass_acc + c : c;   // a group of 64 queries = tiles (t even, t + 1) of this wave (qt0 is a multiple of QT)
            if (fuse.group_counts && (t & 1) && le == 0 && (qt0e + t - 1) * 32 < nq) fuse.group_counts[(size_t)b * ((nq + 63) >> 6) + ((qt0e + t) >> 1)] = pass_acc;
        } else if (he == 0 && q < nq) {
            if (fuse.idx)  // read back by another workgroup of THIS launch: written through to the coherence point (see below)
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(&part[((size_t)b * nsplit + split) * nq + q]),
                                   (unsigned long long)k0 | ((unsigned long long)k1 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                part[((size_t)b * nsplit + split) * nq + q] = make_uint2(k0, k1);
        }
    }
    if (fuse.idx && nsplit > 1) {
        // The last workgroup of this (pair, query block) folds the splits.  No fences: an agent-scope release / acquire pair writes back
        // and INVALIDATES the XCD's L2 -- with a workgroup finishing every few microseconds the train fragments the other workgroups
        // stream would never stay cached (measured: 431 -> 633 us per 64-pair launch).  Instead the partials themselves are relaxed
        // agent-scope atomics (written through / read from the coherence point), every wave waits for its own stores to be acknowledged
        // (vmcnt(0)) before the workgroup's barrier, and only then does thread 0 draw the ticket.
        __shared__ int s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid_end == 0) {
            const int old = __hip_atomic_fetch_add(&fuse.tickets[(size_t)b * qblocks + qb], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = old == nsplit - 1;
            if (s_last) __hip_atomic_store(&fuse.tickets[(size_t)b * qblocks + qb], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (s_last) {
            const uint32_t lmask = (1u << dshift) - 1u;
            const int q_first = qb * NW * QT * 32;
#pragma unroll 1
            for (int rr = 0; rr * (64 * NW) < NW * QT * 32; ++rr) {  // (QT = 1: the first half of the threads)
                const int ql = rr * (64 * NW) + (int)tid_end;
                const int q = ql < NW * QT * 32 ? q_first + ql : nq;
                unsigned long long b0 = ~0ull, b1 = ~0ull;
                auto upd = [&](unsigned long long g) {
                    const bool lt0 = g < b0, lt1 = g < b1;
                    b1 = lt0 ? b0 : (lt1 ? g : b1);
                    b0 = lt0 ? g : b0;
                };
                bool pass = false;
                if (q < nq) {
                    for (int sp = 0; sp < nsplit; ++sp) {
                        const unsigned long long pw = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(&part[((size_t)b * nsplit + sp) * nq + q]),
                                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const uint2 pv = make_uint2((uint32_t)pw, (uint32_t)(pw >> 32));
                        const unsigned long long base = split_tile0 ? 32ull * (unsigned long long)split_tile0[(size_t)b * (nsplit + 1) + sp]
                                                                    : (unsigned long long)sp * rows_per_split;
                        if (pv.x != 0xFFFFFFFFu) upd(((unsigned long long)(pv.x >> dshift) << 32) | (base + (pv.x & lmask)));
                        if (pv.y != 0xFFFFFFFFu) upd(((unsigned long long)(pv.y >> dshift) << 32) | (base + (pv.y & lmask)));
                    }
                    const size_t o = ((size_t)b * nq + q) * fuse.k;
                    const int d0 = (int32_t)(b0 >> 32);
                    fuse.idx[o] = (int32_t)(b0 & 0xFFFFFFFFull);
                    fuse.dist[o] = d0;
                    if (fuse.k == 2) {
                        const int d1 = (int32_t)(b1 >> 32);
                        fuse.idx[o + 1] = (int32_t)(b1 & 0xFFFFFFFFull);
                        fuse.dist[o + 1] = d1;
                        pass = (float)d0 < __fmul_rn(fuse.ratio, (float)d1);
                    } else {
                        pass = true;
                    }
                }
                const int c = __popcll(__ballot(pass));
                const int q_wave = q_first + rr * (64 * NW) + (int)(tid_end & ~63u);   // first query of this wave's 64
                if (fuse.group_counts && le == 0 && q_wave < nq && rr * (64 * NW) + (int)(tid_end & ~63u) < NW * QT * 32) fuse.group_counts[(size_t)b * ((nq + 63) >> 6) + (q_wave >> 6)] = c;
            }
        }
    }
    if (stamps && l_end == 0) clock_stamp(stamps + ((size_t)item * NW + w) * 4, st_c, st_r, ntiles, QT);
    if (fuse.clk && item == 0 && tid_end == 0) {
        fuse.clk[0] = __builtin_amdgcn_s_memtime() - st_c;
        fuse.clk[1] = __builtin_amdgcn_s_memrealtime() - st_r;
        fuse.clk[2] = st_r;
        fuse.clk[3] = fuse.launch_no;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The throughput instance of the LDS-ring kernel (<4, 0, 8, 2, true, false, 4>: eight waves, 128 queries per wave, in-kernel expansion, block
// update of four) on v_mfma_f32_16x16x128_f8f6f4 instead of 32x32x64 (option hamming_mfma_shape = 16).  Work-item mapping, raw ring, LDS-DMA
// copies, barrier protocol, the unrolled pairs with a rolled tail, HammingFuse, tickets, partial table and clock record are those of the
// kernel above; what differs is the tile arithmetic, where a fragment's lanes sit and the epilogue's lane bookkeeping.
//   * Operands: only the symmetric structure of the opcode is used -- for A and B alike lane l holds row / column l & 15 and the 32
//     K-elements of lane group g = l >> 4; D puts column l & 15, rows 4 g + 0..3 into a lane's four registers.  K-half kh covers descriptor
//     words 4 kh .. 4 kh + 3, lane group g takes word 4 kh + g, and a lane's four operand registers are that word's planes 0, 2, 1, 3 (the
//     rule of expand_plane, in both operands).
//   * Fragment ring: same size, and the four ds_read_b128 of a tile keep their addresses; fragment s = 2 rh + kh now holds rows 16 rh + 0..15
//     (row half rh) of K-half kh.  Expansion wave w (word w: kh = w >> 2, g = w & 3) still reads row l >> 1 and forms the plane pair l & 1; it
//     writes two contiguous 256-byte runs (rh = 0, 1) instead of one of 512.
//   * Queries: group u = 0..7 of a wave is queries 32 qt0 + 16 u + (l & 15); bq[u][kh] = the planes of word 4 kh + g.  64 registers as above.
//   * Tile arithmetic per group: two chains of two (one per row half) on 4-register accumulators, interleaved; a lane's eight registers of
//     the two chains -- rows 16 rh + 4 g + 0..3, rh = 0, 1 -- are ONE block of the block rule: g = max8(c0, c1) (three v_max3 and a v_max),
//     m2 = med3(m1, m2, g), m1 = max(m1, g): 6 ops per group, one (c0, c1) pair alive at a time.
//   * Absolute rows: C carries the row within the split, cinit = kAccBias - (32 t + lr) eps for tile t, advanced by -32 eps per tile with four
//     v_pk_add_f32 per wave (all eight groups read it); the running pairs are never re-based and the decode reads the row with frame 0.
//     Magnitudes and fractions: static_asserts at kAccBias.  The ragged tile takes its C from the same running value (rows >= nt: -inf).
//   * Epilogue: a query's keys sit in four lanes (l & 15 equal): top-2 across xor 16 and xor 32; the seven other rows of the best row's block
//     are re-scored, two rows per lane (block_rescan8); lanes of group 0 write; a group of 64 queries = four groups u.
// The MFMAs of a group are written out (the compiler's scheduler puts a chain's two dependent MFMAs back to back); s_nop 7 is the wait the
// compiler itself inserts between this opcode and a VALU read of its result.  The fold keeps the running pair tied to its registers
// (tools/hamming_unit_probe6.hip, tools/hamming_unit_probe7.hip).
// ---------------------------------------------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

// The fused merge of the kernel above (HammingFuse with nsplit > 1: its text, as a function), called by every thread of a workgroup behind
// its partial stores.  QPB = the queries of a workgroup's block, THREADS = its threads; tid_end = the thread's index, le = its lane.
template <int QPB, int THREADS>
__device__ __forceinline__ void fold_splits_by_ticket(const HammingFuse &fuse, uint2 *__restrict__ part, const int32_t *__restrict__ split_tile0, int b, int qb,
                                                      int qblocks, int nsplit, int rows_per_split, int nq, int dshift, unsigned tid_end, int le) {
        // The last workgroup of this (pair, query block) folds the splits.  No fences: an agent-scope release / acquire pair writes back
    // and INVALIDATES the XCD's L2 -- with a workgroup finishing every few microseconds the train fragments the other workgroups
    // stream would never stay cached (measured: 431 -> 633 us per 64-pair launch).  Instead the partials themselves are relaxed
    // agent-scope atomics (written through / read from the coherence point), every wave waits for its own stores to be acknowledged
    // (vmcnt(0)) before the workgroup's barrier, and only then does thread 0 draw the ticket.
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid_end == 0) {
        const int old = __hip_atomic_fetch_add(&fuse.tickets[(size_t)b * qblocks + qb], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == nsplit - 1;
        if (s_last) __hip_atomic_store(&fuse.tickets[(size_t)b * qblocks + qb], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_last) {
        const uint32_t lmask = (1u << dshift) - 1u;
        const int q_first = qb * QPB;
#pragma unroll 1
        for (int rr = 0; rr * THREADS < QPB; ++rr) {  // (QT = 1: the first half of the threads)
            const int ql = rr * THREADS + (int)tid_end;
            const int q = ql < QPB ? q_first + ql : nq;
            unsigned long long b0 = ~0ull, b1 = ~0ull;
            auto upd = [&](unsigned long long g) {
                const bool lt0 = g < b0, lt1 = g < b1;
                b1 = lt0 ? b0 : (lt1 ? g : b1);
                b0 = lt0 ? g : b0;
            };
            bool pass = false;
            if (q < nq) {
                for (int sp = 0; sp < nsplit; ++sp) {
                    const unsigned long long pw = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(&part[((size_t)b * nsplit + sp) * nq + q]),
                                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint2 pv = make_uint2((uint32_t)pw, (uint32_t)(pw >> 32));
                    const unsigned long long base = split_tile0 ? 32ull * (unsigned long long)split_tile0[(size_t)b * (nsplit + 1) + sp]
                                                                : (unsigned long long)sp * rows_per_split;
                    if (pv.x != 0xFFFFFFFFu) upd(((unsigned long long)(pv.x >> dshift) << 32) | (base + (pv.x & lmask)));
                    if (pv.y != 0xFFFFFFFFu) upd(((unsigned long long)(pv.y >> dshift) << 32) | (base + (pv.y & lmask)));
                }
                const size_t o = ((size_t)b * nq + q) * fuse.k;
                const int d0 = (int32_t)(b0 >> 32);
                fuse.idx[o] = (int32_t)(b0 & 0xFFFFFFFFull);
                fuse.dist[o] = d0;
                if (fuse.k == 2) {
                    const int d1 = (int32_t)(b1 >> 32);
                    fuse.idx[o + 1] = (int32_t)(b1 & 0xFFFFFFFFull);
                    fuse.dist[o + 1] = d1;
                    pass = (float)d0 < __fmul_rn(fuse.ratio, (float)d1);
                } else {
                    pass = true;
                }
            }
            const int c = __popcll(__ballot(pass));
            const int q_wave = q_first + rr * THREADS + (int)(tid_end & ~63u);   // first query of this wave's 64
            if (fuse.group_counts && le == 0 && q_wave < nq && rr * THREADS + (int)(tid_end & ~63u) < QPB) fuse.group_counts[(size_t)b * ((nq + 63) >> 6) + (q_wave >> 6)] = c;
        }
    }
}

__device__ __forceinline__ void mfma16_group(const u32x4 (&a)[4], const u32x4 &q0, const u32x4 &q1, const v4f &ci0, const v4f &ci1, v4f &c0, v4f &c1) {
    asm volatile("v_mfma_f32_16x16x128_f8f6f4 %0, %2, %6, %8 cbsz:4 blgp:4\n\t"
                 "v_mfma_f32_16x16x128_f8f6f4 %1, %4, %6, %9 cbsz:4 blgp:4\n\t"
                 "v_mfma_f32_16x16x128_f8f6f4 %0, %3, %7, %0 cbsz:4 blgp:4\n\t"
                 "v_mfma_f32_16x16x128_f8f6f4 %1, %5, %7, %1 cbsz:4 blgp:4\n\t"
                 "s_nop 7"
                 : "=&v"(c0), "=&v"(c1)
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(q0), "v"(q1), "v"(ci0), "v"(ci1));
}
// the maximum of a group's block -- the lane's eight registers of both row halves: three v_max3 and a v_max -- folded into its running pair
__device__ __forceinline__ void top2_update_halves(float &m1, float &m2, const v4f &c0, const v4f &c1) {
    float g = __builtin_fmaxf(__builtin_fmaxf(c0[0], c0[1]), c0[2]);
    g = __builtin_fmaxf(__builtin_fmaxf(g, c0[3]), c1[0]);
    g = __builtin_fmaxf(__builtin_fmaxf(g, c1[1]), c1[2]);
    g = __builtin_fmaxf(g, c1[3]);
    asm volatile("v_med3_f32 %1, %0, %1, %2\n\tv_max_f32 %0, %0, %2" : "+v"(m1), "+v"(m2) : "v"(g));
}
// a query's keys sit in the four lanes with equal l & 15 (disjoint rows): top-2 of the eight keys, in all four lanes
__device__ __forceinline__ uint2 top2_across_groups(const uint32_t (&k)[2]) {
    uint32_t k0 = k[0], k1 = k[1];
#pragma unroll
    for (int x = 16; x <= 32; x <<= 1) {
        const uint32_t o0 = __shfl_xor(k0, x), o1 = __shfl_xor(k1, x);
        k1 = umed3(k0, k1, o0);
        k0 = min(k0, o0);
        k1 = umed3(k0, k1, o1);
        k0 = min(k0, o1);
    }
    return make_uint2(k0, k1);
}
// block_rescan for the block of eight (a lane's eight accumulator registers of a tile: rows T + 16 h + 4 (lane >> 4) + i, h < 2, i < 4): the
// four lanes of a query take i = their group g in both row halves, two rows each; same exclusions, same clamp
__device__ __forceinline__ uint32_t block_rescan8(uint32_t k0, const uint32_t (&q8)[8], const char *rbase, int rows, int dshift, int g) {
    const uint32_t lmask = (1u << dshift) - 1u;
    const int best = (int)(k0 & lmask);
    uint32_t res = 0xFFFFFFFFu;
    uint32_t t2[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const RawRow t = *reinterpret_cast<const RawRow *>(rbase + (size_t)min((best & ~19) + 16 * h + g, rows - 1) * 32);
#pragma unroll
        for (int j = 0; j < 8; ++j) t2[h][j] = t.w[j];
    }
    // (both rows arrive behind one wait: left alone the compiler sinks each load under its row's own condition)
    asm volatile("" ::"v"(t2[0][0]), "v"(t2[0][4]), "v"(t2[1][0]), "v"(t2[1][4]));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = (best & ~19) + 16 * h + g;
        int d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += __popc(t2[h][j] ^ q8[j]);
        const uint32_t key = ((uint32_t)d << dshift) | (uint32_t)r;
        res = (r != best && r < rows && k0 != 0xFFFFFFFFu) ? min(res, key) : res;
    }
    res = min(res, (uint32_t)__shfl_xor(res, 16));
    return min(res, (uint32_t)__shfl_xor(res, 32));
}

__global__ __launch_bounds__(64 * 8, 4) void knn_hamming_mfma_lds16_kernel(
    const uint32_t *__restrict__ qw, size_t q_batch_words, const void *__restrict__ tsrc, size_t t_batch, int nq, int nt,
    int rows_per_split, int nsplit, int dshift, int qblocks, int n_items, uint2 *__restrict__ part,
    unsigned long long *__restrict__ stamps, const int32_t *__restrict__ split_tile0, HammingFuse fuse) {
    constexpr int QT = 4, NG = 2 * QT, NW = 8, PD = 2, KS = 4, NR = 4;
    __shared__ __attribute__((aligned(16))) uint4 ring[2][KS * 64];
    __shared__ __attribute__((aligned(16))) uint32_t raw_ring[NR * 256];
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long st_c = 0, st_r = 0;
    clock_start(stamps || fuse.clk, st_c, st_r);
    const int item = xcd_block_item();
    if (item >= n_items) return;  // workgroup-uniform: no wave of this workgroup reaches a barrier
    const int qb = item % qblocks;
    const int split = (item / qblocks) % nsplit;
    const int b = item / (qblocks * nsplit);
    const int qt0 = (qb * NW + w) * QT;

    u32x4 bq[NG][2];   // the wave's query fragments (filled below, behind the first tile copies)
    v4f cinit[2];   // [row half]: kAccBias - (row within the split) * eps of the tile to come, advanced by -32 eps per tile
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
        for (int i = 0; i < 4; ++i) cinit[rh][i] = kAccBias - (float)(16 * rh + 4 * (l >> 4) + i) * kEps;

    int row0 = split * rows_per_split;
    int row1 = min(nt, row0 + rows_per_split);
    if (split_tile0) {
        row0 = 32 * split_tile0[(size_t)b * (nsplit + 1) + split];
        row1 = min(nt, 32 * split_tile0[(size_t)b * (nsplit + 1) + split + 1]);
    }
    const int tile0 = row0 >> 5;
    const int ntiles = (row1 - row0 + 31) >> 5;

    float m1[NG], m2[NG];
#pragma unroll
    for (int u = 0; u < NG; ++u) m1[u] = m2[u] = -INFINITY;
    v2f pk_step = {-32.0f * kEps, -32.0f * kEps};   // (in a scalar register pair: v_pk_add_f32 takes no literal)
    asm volatile("" : "+s"(pk_step));

    const char *rbase = (const char *)tsrc + ((size_t)b * t_batch + (size_t)tile0 * 32 * (2 * KS)) * 4;   // wave-uniform
    const uint32_t raw_last = (uint32_t)(nt - row0) * (8u * KS) - 4u;   // byte offset of the pair's last train word behind rbase
    // the lane parts of every address of the tile loop, formed once (see the kernel above)
    // (the plane shift l & 1 is bit 3 of xp_plane: with a register of its own the loop takes one more than there are)
    uint32_t xp_frag, xp_raw, xp_plane, xp_voff;
    int xp_it0 = 0;
    auto copy_tile = [&](int t_rel) {
        if (w >= KS) return;  // (wave-uniform: the raw tile is copied by the first KS waves, a quarter each)
        const uint32_t off = min(xp_voff + (uint32_t)(t_rel - PD - xp_it0) * 1024u, raw_last);
        __builtin_amdgcn_global_load_lds((const void *)(rbase + off),
                                         (__attribute__((address_space(3))) void *)&raw_ring[((t_rel + NR - 1) & (NR - 1)) * 256 + w * 64], 4, 0, 0);
    };
    const uint32_t raw_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&raw_ring[0];
    const uint32_t frag_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0];
    {
        const uint32_t lx = (uint32_t)l;
        xp_frag = frag_lds + lx * 16u;
        xp_raw = raw_lds + (uint32_t)w * 4u + (lx >> 1) * 32u;
        // row l >> 1 of word w -> fragment 2 (row >> 4) + (w >> 2), lane 16 (w & 3) + (row & 15), plane pair l & 1
        xp_plane = frag_lds + (lx >> 5) * 2048u + (uint32_t)(w >> 2) * 1024u + (uint32_t)(w & 3) * 256u + (lx & 31u) * 8u;
        xp_voff = PD * 1024u + (uint32_t)w * 256u + lx * 4u;
        asm volatile("" : "+v"(xp_frag), "+v"(xp_raw), "+v"(xp_plane), "+v"(xp_voff));
    }
    auto raw_addr = [&](int t_rel) { return xp_raw + (uint32_t)((t_rel + NR - 1) & (NR - 1)) * 1024u; };   // (raw tile t in slot (t + 3) & 3)
    auto plane_addr = [&](int t_rel) { return xp_plane + (uint32_t)(t_rel & 1) * (KS * 1024u); };
    auto expand_pair = [&](uint32_t x) {
        const uint32_t y = x >> __builtin_amdgcn_ubfe(xp_plane, 3u, 1u);   // dwords 0, 1 = planes 0, 2; dwords 2, 3 = planes 1, 3
        return u32x2{expand_plane0(y, 0x22222222u), expand_plane2(y, 0x22222222u)};
    };
    // the arithmetic of one tile: r[] = the tile's four fragments, c = the tile's C, left as the next tile's
    auto tile_math = [&](const u32x4 (&r)[KS], v4f (&c)[2]) {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            v4f c0, c1;
            mfma16_group(r, bq[u][0], bq[u][1], c[0], c[1], c0, c1);
            top2_update_halves(m1[u], m2[u], c0, c1);
            __builtin_amdgcn_sched_barrier(0);   // (one (c0, c1) pair alive at a time)
        }
        // the next tile's rows: 32 further into the split (four v_pk_add_f32 per wave and tile, for all eight groups)
        const v2f st = pk_step;
        asm volatile("v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %2" : "+v"(c[0].lo), "+v"(c[0].hi) : "s"(st));
        asm volatile("v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %2" : "+v"(c[1].lo), "+v"(c[1].hi) : "s"(st));
    };
    auto tile_body = [&](int it, v4f (&c)[2]) {
        u32x4 r[KS];
        uint32_t x;
        const uint32_t addr = xp_frag + (uint32_t)(it & 1) * (KS * 1024u);
        const uint32_t ra = raw_addr(it + 1), wa = plane_addr(it + 1);
        asm volatile(
            "ds_read_b32 %4, %6\n\tds_read_b128 %0, %5\n\tds_read_b128 %1, %5 offset:1024\n\tds_read_b128 %2, %5 offset:2048\n\t"
            "ds_read_b128 %3, %5 offset:3072"
            : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(x)
            : "v"(addr), "v"(ra)
            : "memory");
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x));
        const u32x2 o = expand_pair(x);
        asm volatile("ds_write_b64 %0, %1" ::"v"(wa), "v"(o) : "memory");
        // (in order behind the four fragment reads: fragment s is complete once at most 4 - s operations are outstanding)
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(r[0]));
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[1]));
        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[2]));
        asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[3]));
        tile_math(r, c);
    };

#pragma unroll
    for (int t = 0; t < PD; ++t)
        if (t < ntiles) copy_tile(t);
    // the query operand, expanded once per wave from the raw descriptors: lane (l & 15, g) owns words g and 4 + g of its row.  Rows >= nq
    // read as zero bits.
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const int row = qt0 * 32 + 16 * u + (l & 15);
        uint32_t v0 = 0u, v1 = 0u;
        if (row < nq) {
            const uint32_t *qp = qw + (size_t)b * q_batch_words + (size_t)row * (2 * KS) + (size_t)(l >> 4);
            v0 = qp[0], v1 = qp[KS];
        }
        bq[u][0] = u32x4{expand_plane(v0, 0), expand_plane(v0, 2), expand_plane(v0, 1), expand_plane(v0, 3)};
        bq[u][1] = u32x4{expand_plane(v1, 0), expand_plane(v1, 2), expand_plane(v1, 1), expand_plane(v1, 3)};
    }
    {
        // tile 0: the query loads' wait has covered the first copies; one barrier makes the four quarters visible, then every wave expands
        // its word of the tile into fragment slot 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        uint32_t x;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(x) : "v"(raw_addr(0)) : "memory");
        const u32x2 o = expand_pair(x);
        asm volatile("ds_write_b64 %0, %1" ::"v"(plane_addr(0)), "v"(o) : "memory");
    }

    // only the last tile of the train set can be ragged; it runs after the loop with the running C, rows >= nt set to -inf (they stay there)
    const bool ragged = row0 + ntiles * 32 > nt;
    const int nfull = ragged ? ntiles - 1 : ntiles;
    auto arrive = [&](int it) {
        // own quarter of raw tile it + 1 landed; own planes of tile `it` (written in the previous iteration, or the prologue) complete
        if (it + PD < ntiles) {
            copy_tile(it + PD);
            asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    };
    int it = 0;
    {
        // steady state, unrolled by the period of the fragment ring: the protocol and the addresses of the kernel above, pair by pair
        const uint32_t dma_lds = raw_lds + (uint32_t)w * 256u;
        int raw_step = 2 * 1024;   // +2 KiB, -2 KiB, ...: the raw slots 0, 1 <-> 2, 3 (scalar)
        auto tile_fixed = [&](auto jc, auto copier) {
            constexpr int J = decltype(jc)::value;
            __builtin_amdgcn_sched_barrier(0);   // (a tile's instructions stay inside the tile, as the back edge of the rolled loop keeps them)
            if constexpr (decltype(copier)::value) {
                const uint32_t m0 = dma_lds + (uint32_t)((it + J + PD + NR - 1) & (NR - 1)) * 1024u - (uint32_t)J * 1024u;
                __builtin_amdgcn_global_load_lds((const void *)(rbase + xp_voff), (__attribute__((address_space(3))) void *)(uintptr_t)m0, 4, J * 1024, 0);
            }
            asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            u32x4 r[KS];
            uint32_t x;
            asm volatile(
                "ds_read_b32 %4, %6 offset:%7\n\tds_read_b128 %0, %5 offset:%8\n\tds_read_b128 %1, %5 offset:%8+1024\n\t"
                "ds_read_b128 %2, %5 offset:%8+2048\n\tds_read_b128 %3, %5 offset:%8+3072"
                : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(x)
                : "v"(xp_frag), "v"(xp_raw), "i"(J * 1024), "i"((J & 1) * (KS * 1024))
                : "memory");
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(x));
            const u32x2 o = expand_pair(x);
            asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(xp_plane), "v"(o), "i"(((J + 1) & 1) * (KS * 1024)) : "memory");
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(r[0]));
            asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r[1]));
            asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r[2]));
            asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r[3]));
            tile_math(r, cinit);
        };
        auto run_pairs = [&](auto copier) {
            while (it + 3 < nfull) {
                tile_fixed(std::integral_constant<int, 0>{}, copier);
                tile_fixed(std::integral_constant<int, 1>{}, copier);
                if constexpr (decltype(copier)::value) xp_voff += 2 * 1024, xp_it0 += 2;
                xp_raw += (uint32_t)raw_step;
                raw_step = -raw_step;
                it += 2;
            }
        };
        if (w < KS) run_pairs(std::true_type{});
        else run_pairs(std::false_type{});
        if (raw_step < 0) xp_raw -= 2 * 1024;   // (back to raw slot 0 for the rolled tail)
    }
    for (; it < nfull; ++it) {
        arrive(it);
        tile_body(it, cinit);
    }
    // what follows the tile loop forms the lane and thread indices anew (see the kernel above)
    const int l_end = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const unsigned tid_end = (unsigned)(w * 64 + l_end);
    if (ragged) {
        arrive(nfull);
#pragma unroll
        for (int rh = 0; rh < 2; ++rh)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int lr = 16 * rh + 4 * (l_end >> 4) + i;
                cinit[rh][i] = (row0 + nfull * 32 + lr < nt) ? cinit[rh][i] : -INFINITY;
            }
        tile_body(nfull, cinit);
    }

    int le = l_end, qt0e = qt0;
    asm volatile("" : "+v"(le), "+s"(qt0e));
    const int ge = le >> 4;
    const float frame = 0.0f;   // (C carries the row within the split)
    int pass_acc = 0;
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        uint32_t k[2];
        const float mm[2] = {m1[u], m2[u]};
#pragma unroll
        for (int j = 0; j < 2; ++j)   // (-inf: no candidate)
            k[j] = mm[j] == -INFINITY ? 0xFFFFFFFFu : decode_key_biased(mm[j], frame, dshift, DistRule{64 * KS, 0, 0});
        const uint2 kk = top2_across_groups(k);
        const int q = qt0e * 32 + 16 * u + (le & 15);
        const uint32_t k0 = kk.x;
        uint32_t k1 = kk.y;
        if (fuse.k != 1) {   // (one neighbour: m1 is exact as it is)
            uint32_t q8[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            if (q < nq) {
                const uint4 *qp = reinterpret_cast<const uint4 *>(qw + (size_t)b * q_batch_words + (size_t)q * (2 * KS));
                const uint4 v0 = qp[0], v1 = qp[1];
                q8[0] = v0.x, q8[1] = v0.y, q8[2] = v0.z, q8[3] = v0.w, q8[4] = v1.x, q8[5] = v1.y, q8[6] = v1.z, q8[7] = v1.w;
            }
            k1 = min(k1, block_rescan8(k0, q8, rbase, nt - row0, dshift, ge));
        }
        if (fuse.idx && nsplit == 1) {  // the final top-2 of the query: outputs straight from the registers
            const uint32_t lmask = (1u << dshift) - 1u;
            bool pass = false;
            if (ge == 0 && q < nq) {
                const size_t o = ((size_t)b * nq + q) * fuse.k;
                const int d0 = k0 == 0xFFFFFFFFu ? -1 : (int)(k0 >> dshift);
                fuse.idx[o] = k0 == 0xFFFFFFFFu ? -1 : (int)(row0 + (k0 & lmask));
                fuse.dist[o] = d0;
                if (fuse.k == 2) {
                    const int d1 = k1 == 0xFFFFFFFFu ? -1 : (int)(k1 >> dshift);
                    fuse.idx[o + 1] = k1 == 0xFFFFFFFFu ? -1 : (int)(row0 + (k1 & lmask));
                    fuse.dist[o + 1] = d1;
                    pass = (float)d0 < __fmul_rn(fuse.ratio, (float)d1);
                } else {
                    pass = true;
                }
            }
            const int c = __popcll(__ballot(pass));
            pass_acc = (u & 3) ? pass_acc + c : c;   // a group of 64 queries = groups 4 j .. 4 j + 3 of this wave (32 qt0 is a multiple of 64)
            if (fuse.group_counts && (u & 3) == 3 && le == 0 && qt0e * 32 + 16 * (u - 3) < nq)
                fuse.group_counts[(size_t)b * ((nq + 63) >> 6) + ((qt0e * 32 + 16 * u) >> 6)] = pass_acc;
        } else if (ge == 0 && q < nq) {
            if (fuse.idx)  // read back by another workgroup of THIS launch: written through to the coherence point
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(&part[((size_t)b * nsplit + split) * nq + q]),
                                   (unsigned long long)k0 | ((unsigned long long)k1 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                part[((size_t)b * nsplit + split) * nq + q] = make_uint2(k0, k1);
        }
    }
    if (fuse.idx && nsplit > 1) fold_splits_by_ticket<NW * QT * 32, 64 * NW>(fuse, part, split_tile0, b, qb, qblocks, nsplit, rows_per_split, nq, dshift, tid_end, le);
    if (stamps && l_end == 0) clock_stamp(stamps + ((size_t)item * NW + w) * 4, st_c, st_r, ntiles, QT);
    if (fuse.clk && item == 0 && tid_end == 0) {
        fuse.clk[0] = __builtin_amdgcn_s_memtime() - st_c;
        fuse.clk[1] = __builtin_amdgcn_s_memrealtime() - st_r;
        fuse.clk[2] = st_r;
        fuse.clk[3] = fuse.launch_no;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The LDS-ring kernel with DYNAMIC train splits.  With fixed, equal work items the hardware's oldest-first arbitration lets the four
// workgroups of a CU finish one after the other (28 ... 50 us for identical items) and the CU runs the second half of the launch
// under-occupied.  Here the workgroups that serve one (image pair, block of 4 query groups, row span) form a TEAM and draw chunks of
// `chunk_tiles` (>= 2) train tiles from the team's counter: a fast workgroup simply takes more chunks, and all of them run dry
// within a chunk of each other.  A workgroup still writes ONE partial top-2 per query (slot = its member index), so the partial
// table and the merge are unchanged; the rows it has seen are not contiguous, so the running pair is re-based by the actual tile
// distance and local rows are relative to the span (<= 8192 rows: (row offset) * 2^-14 < 1/2 keeps rint() exact, see the decode).
// Ring: NB = 3 slots, prefetch distance 1 (the copy of the next tile runs under the current tile's ~2400 cycles).  The chunk after
// the current one is requested (one returning atomic by lane 0 of wave 0, issued BEFORE this iteration's copy so that the iteration's
// own vmcnt wait covers it) at the first tile of every chunk and published to the other waves through LDS behind the barrier.
// The ragged last tile of the train set is the last tile of the last chunk, hence always the last tile of its workgroup.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int QT>
__global__ __launch_bounds__(256, 4) void knn_hamming_mfma_dyn_kernel(
    const uint4 *__restrict__ qfrag, size_t q_batch_u4, const uint4 *__restrict__ tfrag, size_t t_batch_u4, int nq, int nt,
    int span_tiles, int nspan, int nmem, int chunk_tiles, int dshift, int qblocks, int n_items, uint2 *__restrict__ part,
    int *__restrict__ counters, unsigned long long *__restrict__ stamps) {
    constexpr int KS = 4, NB = 3;
    __shared__ __attribute__((aligned(16))) uint4 ring[NB][KS * 64];
    __shared__ int s_claim, s_first;
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long st_c = 0, st_r = 0;
    clock_start(stamps != nullptr, st_c, st_r);
    const int item = xcd_block_item();
    if (item >= n_items) return;  // workgroup-uniform
    const int slots = nspan * nmem;
    const int qb = item % qblocks;
    const int slot_id = (item / qblocks) % slots;
    const int b = item / (qblocks * slots);
    const int span = slot_id / nmem;
    int *ctr = counters + ((size_t)b * qblocks + qb) * nspan + span;
    const int qt0 = (qb * 4 + w) * QT;
    const uint4 *qf = qfrag + (size_t)b * q_batch_u4 + (size_t)qt0 * KS * 64 + l;

    // first chunk (the latency of this one atomic hides under the query fragment loads)
    if (threadIdx.x == 0) s_first = atomicAdd(ctr, 1);

    uint4 bq[QT][KS];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s) bq[t][s] = qf[(size_t)(t * KS + s) * 64];

    const int h = l >> 5;
    const v16f cinit = row_weights(h);

    const int total_tiles = nt >> 5;  // FULL tiles only: the < 32 rows behind them are folded in by the merge kernel
    const int span_tile0 = span * span_tiles;
    const int ntl = min(span_tiles, total_tiles - span_tile0);  // tiles of this span (>= 1)
    const int nchunks = (ntl + chunk_tiles - 1) / chunk_tiles;

    float m1[QT], m2[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) m1[t] = m2[t] = -INFINITY;

    const uint4 *tbase = tfrag + (size_t)b * t_batch_u4 + (size_t)w * 64;  // wave-uniform; tile T at + T * KS * 64
    const uint32_t l16 = (uint32_t)l * 16u;
    auto copy_tile = [&](int tile, int slot) {  // scalar base + 32-bit lane offset
        __builtin_amdgcn_global_load_lds((const void *)(reinterpret_cast<const char *>(tbase + (size_t)tile * KS * 64) + l16),
                                         (__attribute__((address_space(3))) void *)&ring[slot][w * 64], 16, 0, 0);
    };
    const uint32_t ring_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)&ring[0][0];
    auto tile_body = [&](int slot, float rebase) {
        u32x4 r[KS];
        const uint32_t addr = l16 + (ring_base + (uint32_t)slot * (KS * 1024u));
        ring_read_tile(r, addr);
        uint4 a[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = make_uint4(r[s].x, r[s].y, r[s].z, r[s].w);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            v16f acc = mfma_fp4(a[0], bq[t][0], cinit);
#pragma unroll
            for (int s = 1; s < KS; ++s) acc = mfma_fp4(a[s], bq[t][s], acc);
            m1[t] += rebase;  // to this tile's row origin (exact; -inf stays -inf)
            m2[t] += rebase;
#pragma unroll
            for (int reg = 0; reg < 16; reg += 4) top2_update4(m1[t], m2[t], acc[reg], acc[reg + 1], acc[reg + 2], acc[reg + 3]);
            // one accumulator tile alive at a time: without this tie the scheduler interleaves the next unit's MFMA chain on a second
            // accumulator (which buys nothing: MFMA and VALU do not overlap on a SIMD) and pays for it by spilling query fragments.
            // (An empty volatile asm that "rewrites" this unit's result and the next unit's first operand orders the two.)
            asm volatile("" : "+v"(m1[t]), "+v"(m2[t]), "+v"(a[0].x));
        }
    };

    __syncthreads();  // s_first
    int c_cur = __builtin_amdgcn_readfirstlane(s_first);
    int last_tile = span_tile0;  // frame of the decode (stays there when this workgroup got no chunk: everything is -inf)
    if (c_cur < nchunks) {
        int c_nxt = nchunks;  // unknown until requested
        int pos = 0;
        int len = min(chunk_tiles, ntl - c_cur * chunk_tiles);
        int tile = span_tile0 + c_cur * chunk_tiles;
        int prev_tile = tile;
        int slot = 0;
        bool first = true;
        copy_tile(tile, 0);
        for (;;) {
            // request the chunk after this one at the chunk's first tile (not needed when this is the span's last chunk)
            uint32_t req = 0;
            const bool ask = first && (c_cur + 1 < nchunks);
            if (ask && threadIdx.x == 0) {
                const uint32_t zero = 0, one = 1;  // scalar base + zero vector offset: no live 64-bit address register
                asm volatile("global_atomic_add %0, %1, %2, %3 sc0" : "=v"(req) : "v"(zero), "v"(one), "s"(ctr) : "memory");
            }
            // where is the next tile?  inside the chunk, or at the start of the chunk requested one chunk ago
            int next_tile = -1;
            if (pos + 1 < len) next_tile = tile + 1;
            else if (!first && c_nxt < nchunks) next_tile = span_tile0 + c_nxt * chunk_tiles;
            // (first && pos + 1 == len  <=>  a one-tile chunk, which is always the span's last chunk: no next tile)
            const int nslot = slot == NB - 1 ? 0 : slot + 1;
            if (next_tile >= 0) {
                copy_tile(next_tile, nslot);
                asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // this tile's piece (and the atomic, which is older than the copy)
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (ask && threadIdx.x == 0) s_claim = (int)req;
            __builtin_amdgcn_s_barrier();
            tile_body(slot, (float)(32 * (tile - prev_tile)) * kEps);
            last_tile = tile;
            if (ask) c_nxt = __builtin_amdgcn_readfirstlane(s_claim);  // written before this iteration's barrier
            prev_tile = tile;
            if (pos + 1 < len) {
                ++pos;
                ++tile;
                first = false;
            } else if (next_tile >= 0) {
                c_cur = c_nxt;
                c_nxt = nchunks;
                pos = 0;
                len = min(chunk_tiles, ntl - c_cur * chunk_tiles);
                tile = next_tile;
                first = true;
            } else {
                break;
            }
            slot = nslot;
        }
    }

    // decode (frame = the last tile processed): v = (64 KS - 2 d) + (32 (last_tile - span_tile0) - local_row) * eps, |fraction| < 1/2
    const float frame = (float)(32 * (last_tile - span_tile0));
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        uint32_t k[2];
        const float mm[2] = {m1[t], m2[t]};
#pragma unroll
        for (int j = 0; j < 2; ++j)  // (-inf: no candidate)
            k[j] = mm[j] == -INFINITY ? 0xFFFFFFFFu : decode_key(mm[j], frame, dshift, DistRule{64 * KS, 0, 0});
        // (top2_across_halves(k) spelt out: through the helper two scalar copies of the tile loop change places in all three instances)
        const uint32_t o0 = __shfl_xor(k[0], 32), o1 = __shfl_xor(k[1], 32);
        uint32_t k0 = k[0], k1 = k[1];
        k1 = umed3(k0, k1, o0);
        k0 = min(k0, o0);
        k1 = umed3(k0, k1, o1);
        k0 = min(k0, o1);
        const int q = (qt0 + t) * 32 + (l & 31);
        if (h == 0 && q < nq) part[((size_t)b * slots + slot_id) * nq + q] = make_uint2(k0, k1);
    }
    if (stamps && l == 0) clock_stamp(stamps + ((size_t)item * 4 + w) * 4, st_c, st_r, 1, 1);
}

template <int N> using int_c = std::integral_constant<int, N>;

// f(int_c<KS>) for the instantiated K-step count: ks = 1, 2, 4, else 8
template <class F>
void dispatch_ks(int ks, F &&f) {
    switch (ks) {
        case 1: f(int_c<1>{}); break;
        case 2: f(int_c<2>{}); break;
        case 4: f(int_c<4>{}); break;
        default: f(int_c<8>{}); break;
    }
}

// what every instance of the static LDS-ring kernel is launched with (its arguments, in order, behind the grid and the stream)
struct RingLaunch {
    dim3 grid;
    hipStream_t s;
    const uint32_t *qw;
    size_t q_batch_words;
    const void *tsrc;  // train fragments, or the raw train rows for the in-kernel expansion
    size_t t_batch;
    int nq, nt, rps, nsplit, dshift, qblocks, n_items;
    uint2 *part;
    unsigned long long *stamps;
    const int32_t *split_tab;
    HammingFuse fuse;
};
template <int QT, int PRIO, int NW = 4, int PD = 2, bool XP = false, bool ST = false, int BT = 0>
void launch_ring(const RingLaunch &a) {
    hipLaunchKernelGGL((knn_hamming_mfma_lds_kernel<QT, PRIO, NW, PD, XP, ST, BT>), a.grid, dim3(64 * NW), 0, a.s, a.qw, a.q_batch_words, a.tsrc,
                       a.t_batch, a.nq, a.nt, a.rps, a.nsplit, a.dshift, a.qblocks, a.n_items, a.part, a.stamps, a.split_tab, a.fuse);
}

void launch_ring16(const RingLaunch &a) {
    hipLaunchKernelGGL(knn_hamming_mfma_lds16_kernel, a.grid, dim3(64 * 8), 0, a.s, a.qw, a.q_batch_words, a.tsrc, a.t_batch, a.nq, a.nt, a.rps, a.nsplit, a.dshift,
                       a.qblocks, a.n_items, a.part, a.stamps, a.split_tab, a.fuse);
}

// Age-aware split sizes (static LDS-ring kernel).  With exactly R = 4 workgroups per CU the dispatcher deals workgroups breadth
// first, so workgroup L is the (L / num_cus)-th oldest wave set on its CU, and the SIMD arbitrates oldest-first: measured per-tile
// costs with all four ranks active are 1700 / 2100 / 3200 / 5300 cycles (tools/hamming_trace.py), i.e. equal splits finish at
// 62k / 75k / 90k / 105k cycles and the CU runs the second half of the launch under-occupied.  Splits sized by the ranks' rates
// (weights 1/cost) let the four finish together.  Correctness never depends on this: the table only moves split boundaries, and
// it is used only when every query block of a (pair, split) has the same rank.
// For a grid of `grid_x` workgroups over `items` = batch * nsplit * qblocks work items: tab = [batch][nsplit + 1] first tiles of the
// splits (tiles [tab[s], tab[s + 1]) per image pair), or false = not applicable (mixed ranks, or a split above max_rps rows).
bool age_aware_split_table(unsigned grid_x, long long items, int num_cus, int qblocks, int nsplit, int batch, int t_tiles, int max_rps,
                           std::vector<int32_t> &tab) {
    const int per_xcd = (int)(grid_x >> 3);
    tab.assign((size_t)batch * (nsplit + 1), -1);  // first the rank of every (pair, split), then in place its first tile
    for (long long bid = 0; bid < items; ++bid) {  // one workgroup per item; the grid's padding behind them has no work
        const long long item = (bid & 7) * per_xcd + (bid >> 3);
        if (item >= items) continue;
        const int sp = (int)((item / qblocks) % nsplit), bb = (int)(item / ((long long)qblocks * nsplit));
        const int r = (int)(bid / num_cus);
        int32_t &slot = tab[(size_t)bb * (nsplit + 1) + sp];
        if (slot < 0) slot = r;
        else if (slot != r) return false;
    }
    static const double kRate[4] = {1.0 / 1700, 1.0 / 2100, 1.0 / 3200, 1.0 / 5300};
    for (int bb = 0; bb < batch; ++bb) {
        int32_t *h = tab.data() + (size_t)bb * (nsplit + 1);
        double wsum = 0;
        for (int sp = 0; sp < nsplit; ++sp) wsum += kRate[h[sp]];
        int acc_tiles = 0;
        double acc_w = 0;
        for (int sp = 0; sp < nsplit; ++sp) {
            acc_w += kRate[h[sp]];
            h[sp] = acc_tiles;
            int upto = (int)std::llround(t_tiles * acc_w / wsum);
            upto = std::max(upto, acc_tiles + 1);                        // at least one tile per split
            upto = std::min(upto, t_tiles - (nsplit - 1 - sp));          // and one left for every later split
            upto = std::min(upto, acc_tiles + max_rps / 32);          // exact re-basing bound
            acc_tiles = upto;
        }
        h[nsplit] = t_tiles;
        if (t_tiles - h[nsplit - 1] > max_rps / 32) return false;
    }
    return true;
}

}  // namespace

// Called by launch_knn_hamming for descriptors of at most 64 bytes.  qw/tw: word rows (nw words per row, zero padded).
// k, ratio, d_idx, d_dist, d_group_counts: the outputs of the merge step; when the kernel chosen can produce them itself (static LDS-ring
// kernel, QT >= 2) *fused_out = 1 and the caller skips knn_hamming_merge_kernel.
int launch_knn_hamming_mfma(mlpl_ctx *ctx, const uint32_t *qw, size_t q_batch_words, const uint32_t *tw, size_t t_batch_words,
                            int nq, int nt, int nw, int batch, int dshift, hipStream_t s, int *rps_out, int *nsplit_out,
                            int *sps_out, int *tail_row0_out, const int32_t **split_tab_out, uint2 **part_out, int k, float ratio,
                            int32_t *d_idx, int32_t *d_dist, int32_t *d_group_counts, int *fused_out) {
    *fused_out = 0;
    int ks = 1;
    while (ks * 2 < nw) ks *= 2;  // 64-bit K-steps: nw <= 2 -> 1, 4 -> 2, 8 -> 4, 16 -> 8
    if (nw > 16) {
        set_error("knn_hamming (mfma): descriptors above 64 bytes take the VALU kernels");
        return MLPL_E_BAD_INPUT;
    }
    // query tiles per wave: fill the chip first, then amortise the train fragment loads over more queries
    const int nqt = (nq + 31) / 32;
    const int max_qt = ks <= 4 ? 4 : 2;
    int qt = max_qt;
    if (ctx->opt_hamming_mfma_qt > 0) qt = std::min(ctx->opt_hamming_mfma_qt, max_qt);
    while (ctx->opt_hamming_mfma_qt <= 0 && qt > 1 && (long long)((nqt + qt - 1) / qt) * batch < (long long)ctx->num_cus) qt >>= 1;
    const int qgroups = (nqt + qt - 1) / qt;  // wave-level work: one group of qt query tiles against one train split
    const bool lds_ring = ks == 4 && ctx->opt_hamming_mfma_lds != 0;  // workgroup-level work: NW query groups share the train tiles
    const bool dyn = lds_ring && ctx->opt_hamming_mfma_lds == 2 && nt >= 32;  // ... and the train splits are drawn dynamically
    // waves per workgroup of the static ring kernel (option hamming_mfma_waves: 0 = automatic, 4, 8, 16): eight when every wave carries four query
    // tiles (the throughput shape) -- a tile fetched and a barrier passed once per eight waves' units
    const int nwv = (lds_ring && !dyn && qt == 4 && ctx->opt_hamming_mfma_waves != 4) ? (ctx->opt_hamming_mfma_waves == 16 ? 16 : 8) : 4;
    const int qblocks = (qgroups + nwv - 1) / nwv;
    const int q_tiles_padded = lds_ring ? qblocks * nwv * qt : qgroups * qt;
    const int t_tiles = (nt + 31) / 32;

    // train splits: ~4 * opt waves per CU in flight, whole tiles, bounded so that the re-based fraction stays exact
    const int bpc = lds_ring ? std::max(4, ctx->opt_hamming_mfma_blocks_per_cu) : std::max(1, ctx->opt_hamming_mfma_blocks_per_cu);
    const long long target_waves = 4LL * bpc * ctx->num_cus;
    const long long wave_groups = lds_ring ? (long long)nwv * qblocks : (long long)qgroups;
    long long want = (target_waves + wave_groups * batch - 1) / (wave_groups * batch);
    int nsplit = (int)std::max<long long>(1, std::min<long long>(want, t_tiles));
    int rps = ((nt + nsplit - 1) / nsplit + 31) / 32 * 32;
    const int max_rps = ctx->opt_hamming_split_rows == 4096 ? 4096 : kMaxRowsPerSplit;
    rps = std::min(rps, max_rps);
    nsplit = (nt + rps - 1) / rps;
    if (nsplit > 65535) {
        set_error("knn_hamming: train set too large (nt=%d)", nt);
        return MLPL_E_BAD_INPUT;
    }
    // dynamic splits: spans of <= 8192 rows, `nmem` workgroups per (pair, query block, span) drawing chunks of 2 tiles
    int nspan = 1, span_tiles = t_tiles, nmem = 1, sps = 1;
    const int chunk_tiles = 2;
    if (dyn) {
        const int t_full = nt >> 5;  // whole tiles; rows [32 t_full, nt) are folded in by the merge kernel
        nspan = (t_full + 255) / 256;
        span_tiles = (t_full + nspan - 1) / nspan;
        const long long teams = (long long)qblocks * nspan * batch;
        const long long want_mem = ((long long)bpc * ctx->num_cus + teams - 1) / teams;
        nmem = (int)std::max<long long>(1, std::min<long long>(want_mem, (span_tiles + chunk_tiles - 1) / chunk_tiles));
        nsplit = nspan * nmem;
        rps = span_tiles * 32;
        sps = nmem;
        if (nsplit > 65535) {
            set_error("knn_hamming: train set too large (nt=%d)", nt);
            return MLPL_E_BAD_INPUT;
        }
    }
    const long long items = (lds_ring ? (long long)qblocks : (long long)qgroups) * nsplit * batch;  // workgroups (ring) or waves
    if (items > (1LL << 30)) {
        set_error("knn_hamming: problem too large for one launch (nq=%d nt=%d batch=%d)", nq, nt, batch);
        return MLPL_E_BAD_INPUT;
    }

    // Instance of the static LDS-ring kernel.  Precedence (the options do not combine): waves 16 (qt 4 only; the plain <4, 0, 16>) beats a
    // prefetch distance of 4 or 6, which beats prio; prefetch and prio 3 exist at qt 4 with 8 waves only, prio 1 at every shape.  An option
    // the shape has no instance for is ignored: prefetch with 4 waves, prio 3 below 8 waves (prio 0 is run).
    const int pd = (nwv == 8 && (ctx->opt_hamming_mfma_prefetch == 4 || ctx->opt_hamming_mfma_prefetch == 6)) ? ctx->opt_hamming_mfma_prefetch : 2;
    const int prio = (nwv == 16 || pd != 2) ? 0 : ctx->opt_hamming_mfma_prio == 1 ? 1 : (ctx->opt_hamming_mfma_prio == 3 && nwv == 8) ? 3 : 0;
    const int train01 = (lds_ring && !dyn && ctx->opt_hamming_train01) ? 1 : 0;  // {0, +1} train fragments: that kernel only (it has the raw query words)
    // In-kernel expansion of the train tiles (option hamming_expand_inkernel): the throughput instance <4, 0, 8, 2> of the static ring kernel on
    // whole 32-byte rows (a raw tile is then one contiguous KiB) with the +-1 train operand; every other call expands into WS_FRAG_T as before.
    // (The 4-byte LDS-DMA needs word alignment, which a row of uint32_t has.)
    const bool inkernel = ctx->opt_hamming_expand_inkernel && lds_ring && !dyn && nwv == 8 && pd == 2 && prio == 0 && nw == 8 && !train01 &&
                          ((uintptr_t)tw & 3u) == 0;

    // block size of the running top-2 update (option hamming_block_top2): the instances that have the raw train rows
    const int block_top2 = inkernel ? ctx->opt_hamming_block_top2 : 0;
    ctx->dbg_hamming_top2 = block_top2;
    // matrix-core shape (option hamming_mfma_shape): the 16x16x128 form exists for the throughput instance without the stamps trace only
    const int shape = (inkernel && block_top2 == 4 && ctx->opt_hamming_stamps != 1 && ctx->opt_hamming_mfma_shape == 16) ? 16 : 32;
    ctx->dbg_hamming_shape = shape;
    ctx->dbg_hamming_block_rows = shape == 16 ? 8 : block_top2;   // (the 16 shape folds a lane's eight registers of a tile as one block)

    void *qf = nullptr, *tf = nullptr, *part = nullptr;
    int rc;
    const size_t q_u4 = (size_t)q_tiles_padded * ks * 64, t_u4 = (size_t)t_tiles * ks * 64;
    if ((rc = ws_get(ctx, WS_FRAG_Q, (size_t)batch * q_u4 * 16, &qf))) return rc;
    if (!inkernel && (rc = ws_get(ctx, WS_FRAG_T, ((size_t)batch * t_u4 + (size_t)ks * 64) * 16, &tf))) return rc;  // + one spare tile (register prefetch)
    if ((rc = ws_get(ctx, WS_PARTIAL, (size_t)batch * nsplit * nq * sizeof(uint2), &part))) return rc;
    int *counters = nullptr;
    const int counters_per_batch = dyn ? qblocks * nspan : 0;
    if (dyn) {
        void *cp = nullptr;
        if ((rc = ws_get(ctx, WS_COUNTERS, (size_t)batch * counters_per_batch * sizeof(int), &cp))) return rc;
        counters = (int *)cp;
    }
    // the static LDS-ring kernel expands its query operand itself (in registers): only the train set goes through the expansion kernel
    const bool expand_q = !(lds_ring && !dyn);
    const ExpandArgs ta{tw, t_batch_words, nt, t_tiles, (uint4 *)tf};
    const ExpandArgs qa = expand_q ? ExpandArgs{qw, q_batch_words, nq, q_tiles_padded, (uint4 *)qf} : ta;  // blockIdx.z == 0
    const dim3 egrid((unsigned)(((expand_q ? std::max(q_tiles_padded, t_tiles) : t_tiles) * 64 + 255) / 256), batch, expand_q ? 2 : 1);
    // (one thread per K-step when the launch is small: the single-pair latency shape)
    const bool expand_fine = !inkernel && !expand_q && ks == 4 && nw == 8 && !counters && (long long)t_tiles * batch <= 4LL * ctx->num_cus && ctx->opt_hamming_expand_fine;
    if (inkernel) {
        // nothing to expand here: the ring kernel reads the raw train rows
    } else if (expand_fine) {
        hipLaunchKernelGGL(hamming_expand_fine_kernel, dim3((unsigned)t_tiles, batch), dim3(256), 0, s, ta, train01);
    } else {
        dispatch_ks(ks, [&](auto KS) {
            hipLaunchKernelGGL(hamming_expand_kernel<decltype(KS)::value>, egrid, dim3(256), 0, s, qa, ta, nw, counters, counters_per_batch, train01);
        });
    }
    // 1-D grid, remapped in the kernel (XCD-aware); padded so that every XCD gets the same number of workgroups
    const long long blocks = lds_ring ? items : (items + 3) / 4;
    dim3 grid((unsigned)((blocks + 7) / 8 * 8));
    // age-aware split sizes: the table is rebuilt and uploaded only when the shape changes
    const int32_t *split_tab = nullptr;
    std::vector<int32_t> tab;
    if (lds_ring && !dyn && nwv == 4 && ctx->opt_hamming_mfma_weighted && blocks == 4LL * ctx->num_cus && nsplit >= 4 && nsplit <= 256 &&
        batch * (nsplit + 1) <= 4096 && age_aware_split_table(grid.x, items, ctx->num_cus, qblocks, nsplit, batch, t_tiles, max_rps, tab)) {
        const long long key = ((long long)nt << 32) ^ ((long long)nsplit << 20) ^ ((long long)batch << 8) ^ qblocks;
        void *tabp = nullptr;
        if ((rc = ws_get(ctx, WS_SPLIT_TAB, 4096 * sizeof(int32_t), &tabp))) return rc;
        if (ctx->split_tab_key != key || ctx->split_tab_ptr != tabp) {
            // staging in pageable memory of this call (`tab`): the context's pinned block belongs to the entry point that called us (the pair
            // batch entries keep pointers into it across the matching call, and pinned_get frees the block when it grows)
            MLPL_HIP_TRY(hipStreamSynchronize(s));  // the previous table may still be read by kernels in flight
            MLPL_HIP_TRY(hipMemcpyAsync(tabp, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            MLPL_HIP_TRY(hipStreamSynchronize(s));  // the staging vector dies with this call
            ctx->split_tab_key = key;
            ctx->split_tab_ptr = tabp;
        }
        split_tab = (const int32_t *)tabp;
    }
    unsigned long long *stamps = nullptr;
    ctx->dbg_stamp_items = 0;
    if (ctx->opt_hamming_stamps == 1) {
        void *sp = nullptr;
        const long long waves = lds_ring ? items * nwv : items;
        // per-wave records (4 x u64), then a per-tile clock trace of 48 u64 per wave (LDS-ring kernel, static splits)
        if ((rc = ws_get(ctx, WS_DEBUG, (size_t)waves * (32 + 48 * 8), &sp))) return rc;
        MLPL_HIP_TRY(hipMemsetAsync(sp, 0, (size_t)waves * (32 + 48 * 8), s));
        stamps = (unsigned long long *)sp;
        ctx->dbg_stamp_items = (int)waves;
    }
    HammingFuse fuse{nullptr, nullptr, nullptr, nullptr, k, ratio, train01, nullptr, 0ull};
    if (lds_ring && !dyn && ctx->opt_hamming_stamps == 2) {  // clock ring: one 32-byte record per launch, kClockRing launches deep
        void *cp = nullptr;
        if ((rc = ws_get(ctx, WS_CLOCK, (size_t)kClockRing * 32, &cp))) return rc;
        fuse.clk = (unsigned long long *)cp + (size_t)(ctx->hamming_clock_launches % kClockRing) * 4;
        fuse.launch_no = (unsigned long long)ctx->hamming_clock_launches++;
    }
    // (one query tile per wave = a single image pair with sixteen splits: measured with the fused epilogue 26.8 us per pair against 21.2 with
    // the separate merge launch -- the last-arriving workgroup's fold of sixteen written-through partials is a serial tail on a 15 us kernel)
    if (lds_ring && !dyn && qt >= 2 && d_idx && d_dist && (ctx->opt_hamming_fused_merge & 1)) {
        fuse.idx = d_idx, fuse.dist = d_dist, fuse.group_counts = d_group_counts;
        if (nsplit > 1) {  // ticket counters of the (pair, query block)s: zero when (re)allocated, left zero by every launch
            void *tp = nullptr;
            const size_t tb = (size_t)batch * qblocks * sizeof(int);
            if ((rc = ws_get(ctx, WS_TICKETS, tb, &tp))) return rc;   // a slot of its own: nothing else writes it (not the dyn kernel's counters)
            if (ctx->hamming_tickets_ptr != tp || ctx->hamming_tickets_bytes < tb) {
                MLPL_HIP_TRY(hipMemsetAsync(tp, 0, ctx->ws_bytes[WS_TICKETS], s));
                ctx->hamming_tickets_ptr = tp, ctx->hamming_tickets_bytes = ctx->ws_bytes[WS_TICKETS];
            }
            fuse.tickets = (int *)tp;
        }
        *fused_out = 1;
    }
    {
        int *rec = ctx->dbg_hamming_kernel;
        rec[0] = dyn ? 5 : lds_ring ? 4 : 3, rec[1] = (dyn || !lds_ring) ? (ks <= 4 && qt == 4 ? 4 : qt >= 2 ? 2 : 1) : qt;
        rec[2] = (lds_ring && !dyn) ? prio : 0, rec[3] = lds_ring && !dyn ? nwv : 4, rec[4] = lds_ring && !dyn ? pd : 0;
        rec[5] = *fused_out, rec[6] = split_tab != nullptr, rec[7] = expand_fine, rec[8] = nsplit, rec[9] = ks, rec[10] = inkernel;
    }
    prof_mark(ctx, MLPL_PROF_KNN_HAMMING, 0, s);
    if (dyn) {
        auto launch_dyn = [&](auto QT) {
            hipLaunchKernelGGL((knn_hamming_mfma_dyn_kernel<decltype(QT)::value>), grid, dim3(256), 0, s, (const uint4 *)qf, q_u4, (const uint4 *)tf, t_u4, nq,
                               nt, span_tiles, nspan, nmem, chunk_tiles, dshift, qblocks, (int)items, (uint2 *)part, counters, stamps);
        };
        if (qt == 4) launch_dyn(int_c<4>{});
        else if (qt == 2) launch_dyn(int_c<2>{});
        else launch_dyn(int_c<1>{});
    } else if (lds_ring) {
        const RingLaunch ra{grid, s, qw, q_batch_words, inkernel ? (const void *)tw : (const void *)tf, inkernel ? t_batch_words : t_u4, nq, nt, rps, nsplit,
                            dshift, qblocks, (int)items, (uint2 *)part, stamps, split_tab, fuse};
        if (inkernel && stamps)   // (hamming_stamps = 1: the rolled loop with the per-tile clock trace)
            block_top2 == 4 ? launch_ring<4, 0, 8, 2, true, true, 4>(ra) : launch_ring<4, 0, 8, 2, true, true>(ra);
        else if (inkernel)
            block_top2 != 4 ? launch_ring<4, 0, 8, 2, true>(ra) : shape == 16 ? launch_ring16(ra) : launch_ring<4, 0, 8, 2, true, false, 4>(ra);
        else if (nwv == 16) launch_ring<4, 0, 16>(ra);
        else if (nwv == 8 && pd == 4) launch_ring<4, 0, 8, 4>(ra);
        else if (nwv == 8 && pd == 6) launch_ring<4, 0, 8, 6>(ra);
        else if (nwv == 8 && prio == 3) launch_ring<4, 3, 8>(ra);
        else if (nwv == 8 && prio == 1) launch_ring<4, 1, 8>(ra);
        else if (nwv == 8) launch_ring<4, 0, 8>(ra);
        else if (qt == 4) prio == 1 ? launch_ring<4, 1>(ra) : launch_ring<4, 0>(ra);
        else if (qt == 2) prio == 1 ? launch_ring<2, 1>(ra) : launch_ring<2, 0>(ra);
        else prio == 1 ? launch_ring<1, 1>(ra) : launch_ring<1, 0>(ra);
    } else {
        dispatch_ks(ks, [&](auto KS) {
            auto launch_mfma = [&](auto QT) {
                hipLaunchKernelGGL((knn_hamming_mfma_kernel<decltype(KS)::value, decltype(QT)::value>), grid, dim3(256), 0, s, (const uint4 *)qf, q_u4,
                                   (const uint4 *)tf, t_u4, nq, nt, rps, nsplit, dshift, qgroups, (int)items, (uint2 *)part, stamps);
            };
            if constexpr (decltype(KS)::value <= 4) {
                if (qt == 4) return launch_mfma(int_c<4>{});
            }
            if (qt >= 2) launch_mfma(int_c<2>{});
            else launch_mfma(int_c<1>{});
        });
    }
    prof_mark(ctx, MLPL_PROF_KNN_HAMMING, 1, s);
    *rps_out = rps;
    *nsplit_out = nsplit;
    *sps_out = sps;
    *split_tab_out = split_tab;
    *tail_row0_out = dyn ? (nt >> 5) << 5 : nt;
    *part_out = (uint2 *)part;
    return MLPL_OK;
}

}  // namespace mlpl

// subpix.hip -- matchinglib::getSubPixMatches (M/source/matchers.cpp:1085-1297): template-matching sub-pixel refinement of matched keypoints.
// For every match a template of fs x fs pixels (fs odd, 17 ... 255) around keypoint 1 is compared, by the sum of squared differences, at
// 11 x 11 placements in image 2 around keypoint 2; the first minimum of the float32 table is the new integer position and a parabola
// through its four neighbours the sub-pixel offset.  The contract, the declared deviations and the result layouts: include/mlpl_c.h.
//
// One launch.  Grid = (match, list): one 4-wave workgroup per match stages the template and the search window in LDS once (byte loads,
// consecutive lanes on consecutive bytes of an image row; pixels outside the image are written as 0 under a predicate and their address is
// never formed), then lane = placement: threads 0-120 of each half of the workgroup sum every second template row, the template pixels
// read four at a time as a broadcast dword, the window pixels as bytes.  The sums are exact uint32 (255^2 * 255^2 < 2^32), the two halves are
// added, converted once with v_cvt_f32_u32 (round to nearest even) and the minimum is taken over the packed keys (float bits, v * 11 + u):
// the first minimum in row-major order whichever lane holds it.  The workgroup that takes the last ticket of its list runs the list's
// epilogue: counts, status, last-writer-wins keypoint update (index maximum per train keypoint), ordered compaction.
//
// LDS banking (ds_read_u8 / ds_read_b32: bank = dword address mod 32, conflicts within 32-lane halves): 32 consecutive placements touch at
// most four rows of the window, 11 bytes = at most four dwords of each.  window_pitch() picks the row pitch so that one, two and three
// pitches are each at least four banks away from zero: no two rows of a half share a bank.  The template dword is one address per wave.
#include <algorithm>

#include "mlpl_internal.h"

namespace mlpl {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSearch = 11;                  // placements a side
constexpr int kPlacements = kSearch * kSearch;
constexpr int kBorder = 100;                 // the reference's copyMakeBorder
constexpr int kMinSide = 17, kMaxSide = 255;
constexpr int kSubTickets = 16;              // a list's workgroups draw from 16 counters (match index mod 16), the last of each from the list's own
constexpr int kTicketStride = 32;            // ints between counters: one 128-byte line each

enum { DROP_NONE = 0, DROP_BORDER = 1, DROP_SIDE = 2, DROP_COORD = 3 };
enum { F_INLIER = 1, F_REFINED = 2 };        // flag byte: bit 0 inlier, bit 1 refined, bits 2-3 the drop rule

// matchers.cpp:1148-1165 reduced: the larger size (the reference's a > b ? a : b) + 6, at least 18, made odd downwards; 0 = above 255
__host__ __device__ inline int template_side(float size1, float size2) {
    const float m = size1 > size2 ? size1 : size2;
    if (m >= 251.0f) return 0;                       // (int)m + 6 > 256
    const int fs = m >= 12.0f ? (int)m + 6 : 18;     // NaN and everything below 12 stay at the clamp
    return (fs & 1) ? fs : fs - 1;
}
__host__ __device__ inline int template_pitch(int fs) { return (fs + 3) & ~3; }
// bytes per window row: a whole number P of dwords with k * P mod 32 in [4, 28] for k = 1, 2, 3
__host__ __device__ inline int window_pitch(int fs) {
    int p = (fs + 10 + 3) / 4;
    for (;; ++p) {
        bool ok = true;
        for (int k = 1; k <= 3; ++k) {
            const int m = (k * p) & 31;
            ok = ok && m >= 4 && m <= 28;
        }
        if (ok) return 4 * p;
    }
}
__host__ __device__ inline int window_offset(int fs) { return (template_pitch(fs) * fs + 15) & ~15; }
__host__ __device__ inline int lds_bytes(int fs) { return window_offset(fs) + window_pitch(fs) * (fs + 10); }

struct SubpixArgs {
    const mlpl_dmatch *matches;   // [batch][match_stride]; nullptr: match i joins keypoint i of both lists
    const int32_t *n_matches;     // [batch] or nullptr = n_direct
    const float *kp1, *kp2;       // [batch][nq][2], [batch][nt][2]
    const float *size1, *size2;   // [batch][nq], [batch][nt] or nullptr = all 0
    const uint8_t *img1, *img2;
    size_t step1, step2, bstride1, bstride2;
    int w1, h1, w2, h2;
    int match_stride, nq, nt, n_direct, max_side, rule;
    size_t S;                     // row length of the per-match work arrays
    uint32_t *rec;                // [batch][S] flag byte | side << 8
    unsigned long long *pos;      // [batch][S] refined position of keypoint 2 as two floats (refined matches only)
    int32_t *winner;              // [batch][nt] last match of the list that names the train keypoint
    int32_t *tickets;             // [batch][kSubTickets + 1][kTicketStride], zeroed in front of the launch
    int32_t *res;                 // [batch][8] {refined, status, dropped border / side / coordinate, largest side, n_out, inliers}
    mlpl_dmatch *out;
    int32_t *n_out, *status;
    float *kp2_out;               // [batch][nt][2] or nullptr; may be kp2
    uint8_t *inlier;              // [batch][match_stride] or nullptr
};

__device__ inline bool fits_int(float x) { return x >= -2147483648.0f && x < 2147483648.0f; }   // false for NaN

// rows x cols bytes of an image at (x0, y0) into LDS rows of `pitch` bytes; outside the image and in the row padding: 0.  Four loads per
// thread are in flight before the first LDS store: the staging is a chain of global-load latencies, not of bytes.
__device__ inline void stage(uint8_t *dst, int pitch, int rows, int cols, const uint8_t *img, size_t step, int w, int h, int x0, int y0,
                             int tid) {
    constexpr int kInFlight = 4;
    const int total = rows * pitch;
    for (int i0 = tid; i0 < total; i0 += kInFlight * kThreads) {
        uint8_t v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const int i = i0 + k * kThreads;
            const int r = i / pitch, c = i - r * pitch;
            const int x = x0 + c, y = y0 + r;
            v[k] = 0;
            if (i < total && c < cols && x >= 0 && x < w && y >= 0 && y < h) v[k] = img[(size_t)y * step + (size_t)x];
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const int i = i0 + k * kThreads;
            if (i < total) dst[i] = v[k];
        }
    }
}

__global__ __launch_bounds__(kThreads) void subpix_kernel(SubpixArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t s_part[kThreads];
    __shared__ float s_R[kPlacements];
    __shared__ int s_cnt[8];
    __shared__ int s_wsum[kWaves];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x, b = blockIdx.y;
    const int n = std::min(a.n_matches ? std::max(a.n_matches[b], 0) : a.n_direct, a.match_stride);
    const mlpl_dmatch *ml = a.matches ? a.matches + (size_t)b * a.match_stride : nullptr;
    const float *kp1 = a.kp1 + (size_t)b * a.nq * 2, *kp2 = a.kp2 + (size_t)b * a.nt * 2;
    // Per-match results are read back by another workgroup of THIS launch.  As in the fused Hamming epilogue (knn_hamming_mfma.hip) there
    // are no fences -- an agent-scope release / acquire pair per workgroup writes back and invalidates the XCD's L2 and costs more than the
    // matching itself (measured here: 331 -> 236 us per list of 8192 matches at side 17, 13.1 -> 5.9 ms for 64 of them).  The records are
    // relaxed agent-scope atomics (written through to / read from the coherence point), the storing wave waits for their acknowledgement
    // (vmcnt(0)) in front of the workgroup's barrier, and only then does thread 0 draw the ticket.
    uint32_t *rec = a.rec + (size_t)b * a.S;
    unsigned long long *pos = a.pos + (size_t)b * a.S;
    auto put_rec = [&](int j, uint32_t v) { __hip_atomic_store(&rec[j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto get_rec = [&](int j) { return __hip_atomic_load(&rec[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };

    if (i < n) {
        const int q = ml ? std::min(std::max(ml[i].queryIdx, 0), a.nq - 1) : i;
        const int t = ml ? std::min(std::max(ml[i].trainIdx, 0), a.nt - 1) : i;
        const float x1 = kp1[2 * q], y1 = kp1[2 * q + 1], x2 = kp2[2 * t], y2 = kp2[2 * t + 1];
        const float sz1 = a.size1 ? a.size1[(size_t)b * a.nq + q] : 0.0f, sz2 = a.size2 ? a.size2[(size_t)b * a.nt + t] : 0.0f;
        int drop = DROP_NONE, fs = template_side(sz1, sz2);
        if (fs == 0) drop = DROP_SIDE, fs = kMinSide;
        if (fs > a.max_side) drop = DROP_SIDE;
        if (!(fits_int(x1) && fits_int(y1) && fits_int(x2) && fits_int(y2))) drop = DROP_COORD;
        const int d1 = (fs - 1) / 2, d2 = d1 + 5;
        int rx1 = 0, ry1 = 0, rx2 = 0, ry2 = 0;
        if (!drop) {
            // cvRound: round half to even (v_rndne_f32)
            const long long cx1 = (long long)rintf(x1), cy1 = (long long)rintf(y1), cx2 = (long long)rintf(x2), cy2 = (long long)rintf(y2);
            const long long ax = cx1 - d1, ay = cy1 - d1, bx = cx2 - d2, by = cy2 - d2;
            if (ax < -kBorder || ay < -kBorder || ax + fs > (long long)a.w1 + kBorder || ay + fs > (long long)a.h1 + kBorder || bx < -kBorder ||
                by < -kBorder || bx + fs + 10 > (long long)a.w2 + kBorder || by + fs + 10 > (long long)a.h2 + kBorder)
                drop = DROP_BORDER;
            rx1 = (int)ax, ry1 = (int)ay, rx2 = (int)bx, ry2 = (int)by;
        }
        if (drop) {
            if (tid == 0) put_rec(i, (uint32_t)drop << 2);
        } else {
            const int pt = template_pitch(fs), ps = window_pitch(fs);
            uint8_t *T = lds, *W = lds + window_offset(fs);
            stage(T, pt, fs, fs, a.img1 + (size_t)b * a.bstride1, a.step1, a.w1, a.h1, rx1, ry1, tid);
            stage(W, ps, fs + 10, fs + 10, a.img2 + (size_t)b * a.bstride2, a.step2, a.w2, a.h2, rx2, ry2, tid);
            __syncthreads();
            // ---- lane = placement; the two halves of the workgroup take the even and the odd template rows
            const int p = std::min(tid & 127, kPlacements - 1), half = tid >> 7;
            const int v = p / kSearch, u = p - v * kSearch;
            const uint8_t *Wp = W + v * ps + u;
            const int c4n = fs >> 2;
            uint32_t acc = 0;
            for (int r = half; r < fs; r += 2) {
                const uint32_t *Tr = reinterpret_cast<const uint32_t *>(T + r * pt);
                const uint8_t *Wr = Wp + r * ps;
                for (int c4 = 0; c4 < c4n; ++c4) {
                    const uint32_t tw = Tr[c4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int d = (int)Wr[4 * c4 + k] - (int)((tw >> (8 * k)) & 255u);
                        acc += (uint32_t)(d * d);
                    }
                }
                for (int c = 4 * c4n; c < fs; ++c) {
                    const int d = (int)Wr[c] - (int)T[r * pt + c];
                    acc += (uint32_t)(d * d);
                }
            }
            s_part[tid] = acc;
            __syncthreads();
            if (tid < kPlacements) s_R[tid] = __uint2float_rn(s_part[tid] + s_part[tid + 128]);
            __syncthreads();
            if (wave == 0) {
                // ---- first minimum of the float table: minimum of (float bits, placement); the table is non-negative, so the bits order it
                unsigned long long key = ((unsigned long long)__float_as_uint(s_R[lane]) << 32) | (unsigned)lane;
                if (lane + 64 < kPlacements)
                    key = std::min(key, ((unsigned long long)__float_as_uint(s_R[lane + 64]) << 32) | (unsigned)(lane + 64));
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) key = std::min(key, (unsigned long long)__shfl_xor((long long)key, o));
                if (lane == 0) {
                    const int pm = (int)(key & 0xFFFFFFFFull), my = pm / kSearch, mx = pm - my * kSearch;
                    uint32_t f = 0;
                    if ((mx - 5) * (mx - 5) + (my - 5) * (my - 5) <= 16) {   // so mx, my in 1..9: the four neighbours exist
                        f = F_INLIER;
                        const float c = s_R[pm], xp = s_R[pm + 1], xn = s_R[pm - 1], yp = s_R[pm + kSearch], yn = s_R[pm - kSearch];
                        float nx = 2.0f * ((2.0f * c - xn) - xp), ny = 2.0f * ((2.0f * c - yn) - yp);
                        if (nx != 0.0f && ny != 0.0f) {
                            nx = (xp - xn) / nx, ny = (yp - yn) / ny;
                            const float px = (float)(rx2 + mx + d1) + nx, py = (float)(ry2 + my + d1) + ny;
                            __hip_atomic_store(&pos[i], (unsigned long long)__float_as_uint(px) | ((unsigned long long)__float_as_uint(py) << 32),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            f |= F_REFINED;
                        }
                    }
                    put_rec(i, f | ((uint32_t)fs << 8));
                }
            }
        }
    }

    // ---- ticket: the workgroup that finishes a list last runs its epilogue
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        // Two levels: thousands of workgroups of one list are resident at a time, and one counter serialises them on one address
        // (measured: 5.9 -> 3.3 ms for 64 lists of 8192 matches at side 17).
        int32_t *tk = a.tickets + (size_t)b * (kSubTickets + 1) * kTicketStride;
        const int G = (int)gridDim.x, c = i % kSubTickets;
        const int share = (G - c + kSubTickets - 1) / kSubTickets;     // workgroups of this list with the same remainder
        int last = 0;
        if (__hip_atomic_fetch_add(&tk[c * kTicketStride], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == share - 1)
            last = __hip_atomic_fetch_add(&tk[kSubTickets * kTicketStride], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == std::min(G, kSubTickets) - 1;
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- counts and status
    if (tid < 8) s_cnt[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kThreads) {
        const int j = i0 + tid;
        const uint32_t r = j < n ? get_rec(j) : 0u;
        const int f = (int)(r & 255u), sd = (int)(r >> 8);
        const int c_ref = __popcll(__ballot(f & F_REFINED)), c_inl = __popcll(__ballot(f & F_INLIER));
        const int c_b = __popcll(__ballot((f >> 2) == DROP_BORDER)), c_s = __popcll(__ballot((f >> 2) == DROP_SIDE));
        const int c_c = __popcll(__ballot((f >> 2) == DROP_COORD));
        atomicMax(&s_cnt[5], sd);
        if (lane == 0) {
            atomicAdd(&s_cnt[0], c_ref), atomicAdd(&s_cnt[1], c_inl), atomicAdd(&s_cnt[2], c_b), atomicAdd(&s_cnt[3], c_s);
            atomicAdd(&s_cnt[4], c_c);
        }
    }
    __syncthreads();
    const int refined = s_cnt[0], inliers = s_cnt[1];
    const int status = (refined < n / 3 || refined < 2) ? -1 : 0;
    const bool pass = a.rule && status != 0;   // correspondences.cpp:474-477: the list and the keypoints stay as they are

    // ---- keypoints of image 2: every match writes its position to its train keypoint, the last one in list order wins
    if (a.kp2_out) {
        float2 *ko = reinterpret_cast<float2 *>(a.kp2_out) + (size_t)b * a.nt;
        const float2 *ki = reinterpret_cast<const float2 *>(kp2);
        int32_t *win = a.winner + (size_t)b * a.nt;
        if (!pass) {
            for (int j = tid; j < a.nt; j += kThreads) __hip_atomic_store(&win[j], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int j = tid; j < n; j += kThreads) atomicMax(&win[ml ? std::min(std::max(ml[j].trainIdx, 0), a.nt - 1) : j], j);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        for (int j = tid; j < a.nt; j += kThreads) {
            // written by this workgroup's atomics: read where they went, not from a line another list's epilogue left in this CU's L1
            const int w = pass ? -1 : __hip_atomic_load(&win[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            float2 v = ki[j];
            if (w >= 0 && (get_rec(w) & F_REFINED)) {
                const unsigned long long pw = __hip_atomic_load(&pos[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v = make_float2(__uint_as_float((uint32_t)pw), __uint_as_float((uint32_t)(pw >> 32)));
            }
            ko[j] = v;
        }
    }
    if (a.inlier)
        for (int j = tid; j < n; j += kThreads) a.inlier[(size_t)b * a.match_stride + j] = (uint8_t)(get_rec(j) & F_INLIER);

    // ---- the inliers, compacted in list order; under the rule (status 0) in reverse order, as the reference's loop from the end emits them
    if (a.out && ml) {
        mlpl_dmatch *ol = a.out + (size_t)b * a.match_stride;
        int base = 0;
        for (int c0 = 0; c0 < n; c0 += kThreads) {
            const int j = c0 + tid;
            const bool k = j < n && (get_rec(j) & F_INLIER);
            const unsigned long long mask = __ballot(k);
            if (lane == 0) s_wsum[wave] = __popcll(mask);
            __syncthreads();
            int off = base, all = 0;
            for (int w = 0; w < kWaves; ++w) {
                if (w < wave) off += s_wsum[w];
                all += s_wsum[w];
            }
            off += __popcll(mask & ((1ull << lane) - 1ull));
            if (j < n) {
                if (pass) ol[j] = ml[j];
                else if (k) ol[a.rule ? inliers - 1 - off : off] = ml[j];
            }
            base += all;
            __syncthreads();
        }
    }
    if (tid == 0) {
        int32_t *res = a.res + (size_t)b * 8;
        const int n_out = pass ? n : inliers;
        res[0] = refined, res[1] = status, res[2] = s_cnt[2], res[3] = s_cnt[3], res[4] = s_cnt[4], res[5] = s_cnt[5], res[6] = n_out;
        res[7] = inliers;
        if (a.n_out) a.n_out[b] = n_out;
        if (a.status) a.status[b] = status;
    }
}

}  // namespace

int launch_subpix(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, int n_direct,
                  const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2, const uint8_t *d_img1,
                  int width1, int height1, size_t step1, size_t bstride1, const uint8_t *d_img2, int width2, int height2, size_t step2,
                  size_t bstride2, int max_side, int rule, mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status, float *d_kp2_out,
                  uint8_t *d_inlier, SubpixWork *work, hipStream_t s) {
    max_side = max_side <= 0 ? kMaxSide : std::min(std::max(max_side, kMinSide), kMaxSide);
    int lds = 0;
    for (int fs = kMinSide; fs <= max_side; fs += 2) lds = std::max(lds, lds_bytes(fs));
    const size_t S = ((size_t)match_stride + 63) / 64 * 64, B = (size_t)batch;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_rec = 0, o_pos = o_rec + up(B * S * 4), o_win = o_pos + up(B * S * 8),
                 o_res = o_win + up(B * (size_t)nt * 4), o_tick = o_res + up(B * 32), total = o_tick + up(B * (kSubTickets + 1) * kTicketStride * 4);
    void *wsp = nullptr;
    int rc = ws_get(ctx, WS_SUBPIX, total, &wsp);
    if (rc) return rc;
    char *w = static_cast<char *>(wsp);
    SubpixArgs a{};
    a.matches = d_matches, a.n_matches = d_n_matches, a.kp1 = d_kp1, a.kp2 = d_kp2, a.size1 = d_size1, a.size2 = d_size2;
    a.img1 = d_img1, a.img2 = d_img2, a.step1 = step1, a.step2 = step2, a.bstride1 = bstride1, a.bstride2 = bstride2;
    a.w1 = width1, a.h1 = height1, a.w2 = width2, a.h2 = height2;
    a.match_stride = match_stride, a.nq = nq, a.nt = nt, a.n_direct = n_direct, a.max_side = max_side, a.rule = rule;
    a.S = S;
    a.rec = reinterpret_cast<uint32_t *>(w + o_rec);
    a.pos = reinterpret_cast<unsigned long long *>(w + o_pos), a.winner = reinterpret_cast<int32_t *>(w + o_win);
    a.res = reinterpret_cast<int32_t *>(w + o_res), a.tickets = reinterpret_cast<int32_t *>(w + o_tick);
    a.out = d_out, a.n_out = d_n_out, a.status = d_status, a.kp2_out = d_kp2_out, a.inlier = d_inlier;
    MLPL_HIP_TRY(hipMemsetAsync(a.tickets, 0, B * (kSubTickets + 1) * kTicketStride * 4, s));
    MLPL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(subpix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes(kMaxSide)));
    hipLaunchKernelGGL(subpix_kernel, dim3(match_stride, batch), dim3(kThreads), lds, s, a);
    MLPL_HIP_TRY(hipGetLastError());
    if (work) work->res = a.res;
    return MLPL_OK;
}

}  // namespace mlpl

extern "C" int mlpl_subpix_template_side(float size1, float size2) { return mlpl::template_side(size1, size2); }

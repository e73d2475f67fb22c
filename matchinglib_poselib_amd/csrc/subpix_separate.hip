// subpix_separate.hip -- matchinglib::getSubPixMatches_seperate_Imgs (M/source/matchers.cpp:1318-1391): cv::cornerSubPix on the matched
// keypoints of each image on its own.  Every (match, image) is a fixed-point iteration of up to 40 passes over a (2w + 1)^2 window, w = 3 ... 10
// per list and image: sample a (2w + 3)^2 patch bilinearly around the current point, form five masked gradient sums, solve a 2 x 2 system.
// The contract, the summation order, the declared deviations and the result layouts: include/mlpl_c.h.
//
// Two launches.  subpix_sep_window_kernel (one workgroup per list) takes the smallest positive size of the list's matched keypoints of each
// image, writes the two windows and zeroes the list's tickets.  subpix_sep_kernel runs one WAVE per (match, image), two matches per 4-wave
// workgroup, the whole loop inside the launch: the wave stages the (2w + 4)^2 pixels under the patch in LDS (indices clamped to the image:
// edge replication, and no address outside it is ever formed), writes the patch S as floats to LDS, then lane l adds the terms k = l, l + 64,
// ... in double and a __shfl_down halving tree folds the 64 lane sums -- the order the contract names.  All lanes of the wave then carry the
// same five sums and take the same branch.  The waves of a workgroup run different numbers of passes, so inside the loop they only order
// their own LDS traffic (a wave's LDS operations complete in order; the wavefront fence keeps the compiler from moving them) and the
// workgroup barrier comes after the loop.  The workgroup that draws a list's last ticket runs its epilogue, as subpix.hip does: counts,
// status, last-writer-wins keypoint update by an index maximum, ordered or reversed compaction; records cross workgroups as relaxed
// agent-scope atomics.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "mlpl_internal.h"

namespace mlpl {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerGroup = kWaves / 2;        // matches per workgroup
constexpr int kMinW = 3, kMaxW = 10;
constexpr int kProfPitch = 24;               // floats per mask profile row (2 * kMaxW + 1 = 21 used)
constexpr int kPixMax = (2 * kMaxW + 4) * (2 * kMaxW + 4);   // 576 bytes
constexpr int kPatchMax = (2 * kMaxW + 3) * (2 * kMaxW + 3); // 529 floats
constexpr int kMaxIter = 40;
constexpr int kSubTickets = 16;              // as subpix.hip: a list's workgroups draw from 16 counters, the last of each from the list's own
constexpr int kTicketStride = 32;
constexpr int kTicketInts = (kSubTickets + 1) * kTicketStride;

enum { F_INLIER = 1, F_DROP1 = 2, F_DROP2 = 4, F_FAR1 = 8, F_FAR2 = 16 };
enum { R_REFINED = 0, R_STATUS, R_W1, R_W2, R_DROPPED, R_FAR, R_NOUT, R_INLIERS };

__host__ __device__ inline int window_of(float m) {
    m = m > 20.f ? 20.f : m;
    m = m < 6.f ? 6.f : m;
    if (m != m) m = 20.f;       // a NaN passes both clamps; the minimum never is one (it only takes sizes > 0): treated as "no size"
    return (int)ceilf(m / 2.f);
}

struct SepArgs {
    const mlpl_dmatch *matches;   // [batch][match_stride]; nullptr: match i joins keypoint i of both lists
    const int32_t *n_matches;     // [batch] or nullptr = n_direct
    const float *kp1, *kp2;       // [batch][nq][2], [batch][nt][2]
    const float *size1, *size2;   // [batch][nq], [batch][nt] or nullptr
    const uint8_t *img1, *img2;
    size_t step1, step2, bstride1, bstride2;
    int w1, h1, w2, h2;
    int match_stride, nq, nt, n_direct, rule;
    const float *profiles;        // [8][kProfPitch] mask profiles of w = 3 ... 10
    size_t S;                     // row length of the per-match work arrays
    uint32_t *rec;                // [batch][S] flag byte
    unsigned long long *pos1, *pos2;   // [batch][S] refined positions as two floats (inliers only)
    int32_t *winner1, *winner2;   // [batch][nq], [batch][nt] last match of the list that names the keypoint
    int32_t *tickets;             // [batch][kTicketInts], zeroed by the window kernel
    int32_t *res;                 // [batch][8], R_*
    int32_t *iters;               // [batch][match_stride][2] or nullptr
    mlpl_dmatch *out;
    int32_t *n_out, *status;
    float *kp1_out, *kp2_out;     // [batch][nq][2] / [batch][nt][2] or nullptr; may be kp1 / kp2
    uint8_t *inlier;              // [batch][match_stride] or nullptr
};

__device__ inline int list_length(const SepArgs &a, int b) {
    return std::min(a.n_matches ? std::max(a.n_matches[b], 0) : a.n_direct, a.match_stride);
}

__global__ __launch_bounds__(kThreads) void subpix_sep_window_kernel(SepArgs a) {
    __shared__ float s_min[kWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int n = list_length(a, b);
    const mlpl_dmatch *ml = a.matches ? a.matches + (size_t)b * a.match_stride : nullptr;
    float m1 = FLT_MAX, m2 = FLT_MAX;
    for (int i = tid; i < n; i += kThreads) {
        const int q = ml ? std::min(std::max(ml[i].queryIdx, 0), a.nq - 1) : i;
        const int t = ml ? std::min(std::max(ml[i].trainIdx, 0), a.nt - 1) : i;
        if (a.size1) {
            const float s = a.size1[(size_t)b * a.nq + q];
            if (s > 0.f && s < m1) m1 = s;
        }
        if (a.size2) {
            const float s = a.size2[(size_t)b * a.nt + t];
            if (s > 0.f && s < m2) m2 = s;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m1 = fminf(m1, __shfl_xor(m1, o)), m2 = fminf(m2, __shfl_xor(m2, o));
    if (lane == 0) s_min[wave][0] = m1, s_min[wave][1] = m2;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWaves; ++w) m1 = fminf(m1, s_min[w][0]), m2 = fminf(m2, s_min[w][1]);
        a.res[(size_t)b * 8 + R_W1] = window_of(m1);
        a.res[(size_t)b * 8 + R_W2] = window_of(m2);
    }
    for (int i = tid; i < kTicketInts; i += kThreads) a.tickets[(size_t)b * kTicketInts + i] = 0;
}

__device__ inline bool fits_int(float x) { return x >= -2147483648.0f && x < 2147483648.0f; }   // false for NaN

// orders this wave's LDS stores in front of its later LDS loads (other lanes' data); the hardware completes a wave's LDS operations in order
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// idx / d for idx < 1024, d in [7, 24] with inv = 65536 / d + 1: exact while idx * (inv * d - 65536) < 65536, and inv * d - 65536 <= d
__device__ inline int div_small(int idx, int inv) { return (idx * inv) >> 16; }

// folds the 64 lane values: v[l] += v[l + s] for s = 32 ... 1; lane 0 holds the result, returned to every lane
__device__ inline double wave_fold(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s);
    return __shfl(v, 0);
}

struct Refined {
    float x, y;
    int iters, far;
};

// cv::cornerSubPix on one point by one wave; pix / S / g: this wave's LDS
__device__ inline Refined refine_point(const uint8_t *img, size_t step, int cols, int rows, float tx, float ty, int w, const float *prof,
                                       uint8_t *pix, float *S, float *g, int lane) {
    const int W = 2 * w + 1, SS = W + 2, PS = W + 3;
    const int invW = 65536 / W + 1, invSS = 65536 / SS + 1, invPS = 65536 / PS + 1;
    if (lane < W) g[lane] = prof[(w - kMinW) * kProfPitch + lane];
    float cx = tx, cy = ty;
    int iter = 0;
    bool nonfinite = false;
    for (;;) {
        // ---- a. sampling
        const float sx = cx - (float)(w + 1), sy = cy - (float)(w + 1);
        const float fx = floorf(sx), fy = floorf(sy);
        const float fa = sx - fx, fb = sy - fy;
        // the first pass may start outside the image: beyond these bounds every clamped index is the same
        const int ix = (int)fminf(fmaxf(fx, -64.f), (float)(cols + 64)), iy = (int)fminf(fmaxf(fy, -64.f), (float)(rows + 64));
        const float a11 = (1.f - fa) * (1.f - fb), a12 = fa * (1.f - fb), a21 = (1.f - fa) * fb, a22 = fa * fb;
        wave_lds_sync();   // the previous pass has read pix and S (and g is written)
        for (int idx = lane; idx < PS * PS; idx += 64) {
            const int r = div_small(idx, invPS), c = idx - r * PS;
            const int y = std::min(std::max(iy + r, 0), rows - 1), x = std::min(std::max(ix + c, 0), cols - 1);
            pix[idx] = img[(size_t)y * step + (size_t)x];
        }
        wave_lds_sync();
        for (int idx = lane; idx < SS * SS; idx += 64) {
            const int r = div_small(idx, invSS), c = idx - r * SS;
            const uint8_t *p = pix + r * PS + c;
            S[idx] = (((float)p[0] * a11 + (float)p[1] * a12) + (float)p[PS] * a21) + (float)p[PS + 1] * a22;
        }
        wave_lds_sync();
        // ---- b, c. the five sums: lane l adds k = l, l + 64, ... starting from its first term, then the halving tree
        double va = 0.0, vb = 0.0, vc = 0.0, v1 = 0.0, v2 = 0.0;
        for (int k = lane, first = 1; k < W * W; k += 64, first = 0) {
            const int i = div_small(k, invW), j = k - i * W;
            const float *s = S + (i + 1) * SS + (j + 1);
            const double tgx = (double)s[1] - (double)s[-1], tgy = (double)s[SS] - (double)s[-SS];
            const double m = (double)(g[i] * g[j]);
            const double gxx = (tgx * tgx) * m, gxy = (tgx * tgy) * m, gyy = (tgy * tgy) * m;
            const double px = (double)(j - w), py = (double)(i - w);
            const double t1 = gxx * px + gxy * py, t2 = gxy * px + gyy * py;
            if (first) va = gxx, vb = gxy, vc = gyy, v1 = t1, v2 = t2;
            else va = va + gxx, vb = vb + gxy, vc = vc + gyy, v1 = v1 + t1, v2 = v2 + t2;
        }
        const double A = wave_fold(va), B = wave_fold(vb), C = wave_fold(vc), bb1 = wave_fold(v1), bb2 = wave_fold(v2);
        // ---- d. singular system
        const double det = A * C - B * B;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
        // ---- e. update
        const double scale = 1.0 / det;
        const float nx = (float)(((double)cx + (C * scale) * bb1) - (B * scale) * bb2);
        const float ny = (float)(((double)cy - (B * scale) * bb1) + (A * scale) * bb2);
        if (!(fabsf(nx) <= FLT_MAX && fabsf(ny) <= FLT_MAX)) {
            nonfinite = true;
            break;
        }
        const float ex = nx - cx, ey = ny - cy;
        const float err = ex * ex + ey * ey;
        cx = nx, cy = ny;
        // ---- f. leaving the image
        if (cx < 0.f || cx >= (float)cols || cy < 0.f || cy >= (float)rows) break;
        // ---- g. termination
        if (!(++iter < kMaxIter && (double)err > 1e-6)) break;
    }
    Refined r{cx, cy, iter, 0};
    if (nonfinite) r.x = tx, r.y = ty;
    else if (fabsf(cx - tx) > (float)w || fabsf(cy - ty) > (float)w) r.x = tx, r.y = ty, r.far = 1;
    return r;
}

__global__ __launch_bounds__(kThreads) void subpix_sep_kernel(SepArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pix[kWaves][kPixMax];
    __shared__ float s_S[kWaves][kPatchMax + 3];
    __shared__ float s_g[kWaves][kProfPitch];
    __shared__ float s_xy[kWaves][2];
    __shared__ int s_flag[kWaves][2];      // {dropped, far}
    __shared__ int s_cnt[4];
    __shared__ int s_wsum[kWaves];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int i = blockIdx.x * kPerGroup + (wave >> 1), image = wave & 1;
    const int n = list_length(a, b);
    const mlpl_dmatch *ml = a.matches ? a.matches + (size_t)b * a.match_stride : nullptr;
    const float *kp1 = a.kp1 + (size_t)b * a.nq * 2, *kp2 = a.kp2 + (size_t)b * a.nt * 2;
    // Per-match results are read back by another workgroup of THIS launch: relaxed agent-scope atomics, acknowledged (vmcnt(0)) in front
    // of the workgroup's barrier, and only then does thread 0 draw the ticket (subpix.hip has the measurements behind this form).
    uint32_t *rec = a.rec + (size_t)b * a.S;
    unsigned long long *pos1 = a.pos1 + (size_t)b * a.S, *pos2 = a.pos2 + (size_t)b * a.S;
    auto put_rec = [&](int j, uint32_t v) { __hip_atomic_store(&rec[j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto get_rec = [&](int j) { return __hip_atomic_load(&rec[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto put_pos = [&](unsigned long long *p, int j, float x, float y) {
        __hip_atomic_store(&p[j], (unsigned long long)__float_as_uint(x) | ((unsigned long long)__float_as_uint(y) << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    };
    auto get_pos = [&](const unsigned long long *p, int j) {
        const unsigned long long v = __hip_atomic_load(&p[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return make_float2(__uint_as_float((uint32_t)v), __uint_as_float((uint32_t)(v >> 32)));
    };

    float ox = 0.f, oy = 0.f;   // this wave's point as it came
    if (i < n) {
        const int k = image == 0 ? (ml ? std::min(std::max(ml[i].queryIdx, 0), a.nq - 1) : i)
                                 : (ml ? std::min(std::max(ml[i].trainIdx, 0), a.nt - 1) : i);
        const float *kp = image == 0 ? kp1 : kp2;
        ox = kp[2 * k], oy = kp[2 * k + 1];
        const int w = std::min(std::max(a.res[(size_t)b * 8 + (image == 0 ? R_W1 : R_W2)], kMinW), kMaxW);
        Refined r{ox, oy, 0, 0};
        const bool dropped = !(fits_int(ox) && fits_int(oy));
        if (!dropped)
            r = image == 0 ? refine_point(a.img1 + (size_t)b * a.bstride1, a.step1, a.w1, a.h1, ox, oy, w, a.profiles, s_pix[wave], s_S[wave],
                                          s_g[wave], lane)
                           : refine_point(a.img2 + (size_t)b * a.bstride2, a.step2, a.w2, a.h2, ox, oy, w, a.profiles, s_pix[wave], s_S[wave],
                                          s_g[wave], lane);
        if (lane == 0) {
            s_xy[wave][0] = r.x, s_xy[wave][1] = r.y, s_flag[wave][0] = dropped ? 1 : 0, s_flag[wave][1] = r.far;
            if (a.iters) a.iters[((size_t)b * a.match_stride + i) * 2 + image] = r.iters;
        }
    }
    __syncthreads();
    if (i < n && image == 1 && lane == 0) {
        // ---- the match: this is wave 2 m + 1, its partner 2 m holds point 1
        const float x1 = s_xy[wave - 1][0], y1 = s_xy[wave - 1][1], x2 = s_xy[wave][0], y2 = s_xy[wave][1];
        const int q = ml ? std::min(std::max(ml[i].queryIdx, 0), a.nq - 1) : i;
        const float o1x = kp1[2 * q], o1y = kp1[2 * q + 1];
        const float e1x = o1x - x1, e1y = o1y - y1, e2x = ox - x2, e2y = oy - y2;
        const float d1 = e1x * e1x + e1y * e1y, d2 = e2x * e2x + e2y * e2y;
        uint32_t f = (s_flag[wave - 1][0] ? F_DROP1 : 0) | (s_flag[wave][0] ? F_DROP2 : 0) | (s_flag[wave - 1][1] ? F_FAR1 : 0) |
                     (s_flag[wave][1] ? F_FAR2 : 0);
        if (!(f & (F_DROP1 | F_DROP2)) && !(d1 > 12.f || d2 > 12.f)) {
            f |= F_INLIER;
            put_pos(pos1, i, x1, y1);
            put_pos(pos2, i, x2, y2);
        }
        put_rec(i, f);
    }

    // ---- ticket: the workgroup that finishes a list last runs its epilogue
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        int32_t *tk = a.tickets + (size_t)b * kTicketInts;
        const int G = (int)gridDim.x, c = (int)blockIdx.x % kSubTickets;
        const int share = (G - c + kSubTickets - 1) / kSubTickets;     // workgroups of this list with the same remainder
        int last = 0;
        if (__hip_atomic_fetch_add(&tk[c * kTicketStride], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == share - 1)
            last = __hip_atomic_fetch_add(&tk[kSubTickets * kTicketStride], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == std::min(G, kSubTickets) - 1;
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- counts and status
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kThreads) {
        const int j = i0 + tid;
        const uint32_t f = j < n ? get_rec(j) : 0u;
        const int c_inl = __popcll(__ballot(f & F_INLIER));
        const int c_drop = __popcll(__ballot(f & F_DROP1)) + __popcll(__ballot(f & F_DROP2));
        const int c_far = __popcll(__ballot(f & F_FAR1)) + __popcll(__ballot(f & F_FAR2));
        if (lane == 0) atomicAdd(&s_cnt[0], c_inl), atomicAdd(&s_cnt[1], c_drop), atomicAdd(&s_cnt[2], c_far);
    }
    __syncthreads();
    const int refined = s_cnt[0];
    const int status = (refined < n / 3 || refined < 2) ? -1 : 0;
    const bool pass = a.rule && status != 0;   // correspondences.cpp:474-477: the list and the keypoints stay as they are

    // ---- keypoints: every match writes its position to its keypoint, the last one in list order wins.  Under the rule the reference's
    // caller never takes the refined keypoints 1 (correspondences.cpp:480-483): a plain copy.
    for (int side = 0; side < 2; ++side) {
        float *out = side == 0 ? a.kp1_out : a.kp2_out;
        if (!out) continue;
        const int nk = side == 0 ? a.nq : a.nt;
        float2 *ko = reinterpret_cast<float2 *>(out) + (size_t)b * nk;
        const float2 *ki = reinterpret_cast<const float2 *>(side == 0 ? kp1 : kp2);
        int32_t *win = (side == 0 ? a.winner1 : a.winner2) + (size_t)b * nk;
        const unsigned long long *pos = side == 0 ? pos1 : pos2;
        const bool copy = pass || (side == 0 && a.rule);
        if (!copy) {
            for (int j = tid; j < nk; j += kThreads) __hip_atomic_store(&win[j], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int j = tid; j < n; j += kThreads) {
                const int k = !ml ? j : side == 0 ? std::min(std::max(ml[j].queryIdx, 0), nk - 1) : std::min(std::max(ml[j].trainIdx, 0), nk - 1);
                atomicMax(&win[k], j);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        for (int j = tid; j < nk; j += kThreads) {
            const int w = copy ? -1 : __hip_atomic_load(&win[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            float2 v = ki[j];
            if (w >= 0 && (get_rec(w) & F_INLIER)) v = get_pos(pos, w);
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
                else if (k) ol[a.rule ? refined - 1 - off : off] = ml[j];
            }
            base += all;
            __syncthreads();
        }
    }
    if (tid == 0) {
        int32_t *res = a.res + (size_t)b * 8;
        const int n_out = pass ? n : refined;
        res[R_REFINED] = refined, res[R_STATUS] = status, res[R_DROPPED] = s_cnt[1], res[R_FAR] = s_cnt[2], res[R_NOUT] = n_out;
        res[R_INLIERS] = refined;
        if (a.n_out) a.n_out[b] = n_out;
        if (a.status) a.status[b] = status;
    }
}

// g[i] = (float)exp(-(double)(y * y)), float y = (float)(i - w) / w, rows w = 3 ... 10
void mask_profiles(float *p) {
    for (int w = kMinW; w <= kMaxW; ++w)
        for (int i = 0; i < kProfPitch; ++i) {
            const float y = (float)(i - w) / (float)w;
            p[(w - kMinW) * kProfPitch + i] = i <= 2 * w ? (float)std::exp(-(double)(y * y)) : 0.f;
        }
}

}  // namespace

int subpix_separate_init(mlpl_ctx *ctx) {
    void *prof = nullptr;
    const int rc = ws_get(ctx, WS_SUBPIX_SEP_MASK, sizeof(float) * 8 * kProfPitch, &prof);
    if (rc) return rc;
    float host[8 * kProfPitch];
    mask_profiles(host);
    MLPL_HIP_TRY(hipMemcpy(prof, host, sizeof(host), hipMemcpyHostToDevice));
    ctx->subpix_sep_mask_ptr = prof;
    return MLPL_OK;
}

int launch_subpix_separate(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, int n_direct,
                           const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2,
                           const uint8_t *d_img1, int width1, int height1, size_t step1, size_t bstride1, const uint8_t *d_img2, int width2,
                           int height2, size_t step2, size_t bstride2, int rule, mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status,
                           float *d_kp1_out, float *d_kp2_out, uint8_t *d_inlier, int32_t *d_iters, SubpixWork *work, hipStream_t s) {
    const void *prof = ctx->subpix_sep_mask_ptr;   // uploaded by mlpl_ctx_create (subpix_separate_init)
    if (!prof) {
        set_error("subpix_separate: the context holds no mask profiles");
        return MLPL_E_BAD_INPUT;
    }
    int rc;
    const size_t S = ((size_t)match_stride + 63) / 64 * 64, B = (size_t)batch;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_rec = 0, o_pos1 = o_rec + up(B * S * 4), o_pos2 = o_pos1 + up(B * S * 8), o_win1 = o_pos2 + up(B * S * 8),
                 o_win2 = o_win1 + up(B * (size_t)nq * 4), o_res = o_win2 + up(B * (size_t)nt * 4), o_tick = o_res + up(B * 32),
                 total = o_tick + up(B * kTicketInts * 4);
    void *wsp = nullptr;
    if ((rc = ws_get(ctx, WS_SUBPIX_SEP, total, &wsp))) return rc;
    char *w = static_cast<char *>(wsp);
    SepArgs a{};
    a.matches = d_matches, a.n_matches = d_n_matches, a.kp1 = d_kp1, a.kp2 = d_kp2, a.size1 = d_size1, a.size2 = d_size2;
    a.img1 = d_img1, a.img2 = d_img2, a.step1 = step1, a.step2 = step2, a.bstride1 = bstride1, a.bstride2 = bstride2;
    a.w1 = width1, a.h1 = height1, a.w2 = width2, a.h2 = height2;
    a.match_stride = match_stride, a.nq = nq, a.nt = nt, a.n_direct = n_direct, a.rule = rule;
    a.profiles = static_cast<const float *>(prof);
    a.S = S;
    a.rec = reinterpret_cast<uint32_t *>(w + o_rec);
    a.pos1 = reinterpret_cast<unsigned long long *>(w + o_pos1), a.pos2 = reinterpret_cast<unsigned long long *>(w + o_pos2);
    a.winner1 = reinterpret_cast<int32_t *>(w + o_win1), a.winner2 = reinterpret_cast<int32_t *>(w + o_win2);
    a.res = reinterpret_cast<int32_t *>(w + o_res), a.tickets = reinterpret_cast<int32_t *>(w + o_tick);
    a.iters = d_iters;
    a.out = d_out, a.n_out = d_n_out, a.status = d_status, a.kp1_out = d_kp1_out, a.kp2_out = d_kp2_out, a.inlier = d_inlier;
    hipLaunchKernelGGL(subpix_sep_window_kernel, dim3(batch), dim3(kThreads), 0, s, a);
    MLPL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(subpix_sep_kernel, dim3((match_stride + kPerGroup - 1) / kPerGroup, batch), dim3(kThreads), 0, s, a);
    MLPL_HIP_TRY(hipGetLastError());
    if (work) work->res = a.res;
    return MLPL_OK;
}

}  // namespace mlpl

extern "C" int mlpl_subpix_separate_window(float min_size) { return mlpl::window_of(min_size); }

// gms.hip -- the GMS match filter (grid-based motion statistics: matchinglib::filterMatchesGMS, M/source/gms.cpp over
// M/thirdparty/gms-1.0/src/MatchGMS.cpp) on gfx950.  One workgroup per match list; one launch runs every (scale, rotation) run and the four
// grid types of each.  Everything is integer voting on a 20 x 20 left grid, so every result is reproducible bit for bit.
//
// What the kernel uses of the reference's structure:
//   * the cell of a match depends on the grid type (left) and the scale level (right) only, so the 4 + 5 cell codes per match are computed
//     once, in the reference's float arithmetic (reciprocal, one multiply, a separately rounded + 0.5f);
//   * the motion statistics, the point counts and the partner cell (first row maximum) depend on (scale, grid type) but not on the rotation
//     type; only the 3 x 3 neighbourhood score does.  A (scale, grid type) step therefore serves all eight rotation types: a match carries one
//     inlier bit per rotation type, and the run counts of a scale level are eight bit counts;
//   * the dense 400 x (Wr Hr) table is never formed.  A step buckets the matches by left cell (400-bin LDS histogram, scan, scatter of the
//     uint16 right cells); one wave per left cell finds the row's first maximum in a per-wave right-cell histogram (reduction on
//     (count, lowest index)) and counts the 9 x 9 terms motion[left neighbour][right neighbour of the partner] inside the neighbour buckets.
// Every quantity is a count, so the order of the atomics reaches no result.
#include <algorithm>

#include "mlpl_internal.h"

namespace mlpl {

namespace {

constexpr int kThreads = 512, kWaves = 8, kGrid = 20, kCells = 400, kMaxRight = 1600, kScales = 5;
// (int)(20 * ratio) for the ratios 1, 1/2, 1/sqrt 2, sqrt 2, 2
__device__ const int kRightSize[kScales] = {20, 10, 14, 28, 40};
// the eight outer cells of a 3 x 3 block in clockwise order, and the position of a cell in that ring; rotation type r moves the ring by r steps
__device__ const int kRing[8] = {0, 1, 2, 5, 8, 7, 6, 3};
__device__ const int kRingPos[9] = {0, 1, 2, 7, 0, 3, 6, 5, 4};

constexpr int kCodeRefDrop = -1;   // the reference drops the match (a negative index)
constexpr int kCodeDevDrop = -2;   // the reference would read or write out of bounds or convert an unrepresentable float: dropped here

struct GmsArgs {
    const mlpl_dmatch *matches;   // [batch][match_stride]
    const int32_t *n_matches;     // [batch], or nullptr: n_direct
    const float *kp1, *kp2;       // [batch][nq][2], [batch][nt][2]
    int match_stride, nq, nt, n_direct, n_scales, rot_mask, rule;
    float winv1, hinv1, winv2, hinv2;
    size_t S;                     // workspace matches per problem (a multiple of 64)
    int16_t *codes;               // [batch][9][S]: left cell at grid types 1-4, right cell at scale levels 0-4
    uint16_t *bucket;             // [batch][S]: right cells ordered by left cell
    uint8_t *drop, *flags, *keep; // [batch][S]
    int32_t *res;                 // [batch][8] = {count, scale level, rotation type, dropped by the out-of-bounds rule, n_out, 0, 0, 0}
    mlpl_dmatch *out;
    int32_t *n_out, *n_inliers;
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool fits_int(float v) { return v >= -2147483648.0f && v < 2147483648.0f; }   // false for NaN and infinities

__device__ __forceinline__ int left_code(float fx, float fy) {
    const float flx = floorf(fx), fly = floorf(fy);
    if (!fits_int(flx) || !fits_int(fly)) return kCodeDevDrop;
    const int x = (int)flx, y = (int)fly;
    if (x >= kGrid || y >= kGrid) return kCodeRefDrop;
    const long long idx = (long long)x + (long long)kGrid * y;   // a negative x is not checked: it aliases into the row before
    return idx < 0 ? kCodeRefDrop : (int)idx;
}

__device__ __forceinline__ int right_code(float xn, float yn, int W) {
    const float flx = floorf(__fmul_rn(xn, (float)W)), fly = floorf(__fmul_rn(yn, (float)W));
    if (!fits_int(flx) || !fits_int(fly)) return kCodeDevDrop;
    const long long idx = (long long)(int)flx + (long long)W * (int)fly;   // no bounds check on x or y in the reference
    if (idx < 0) return kCodeRefDrop;
    return idx >= (long long)W * W ? kCodeDevDrop : (int)idx;
}

// score < 6 sqrt(thresh / numPair) in double; off the exact tie the comparison of integers decides the same way
__device__ __forceinline__ bool gms_reject(int score, int thresh, int num_pair) {
    const long long lhs = (long long)score * score * num_pair, rhs = 36ll * thresh;
    if (lhs != rhs) return lhs < rhs;
    const double t = __dmul_rn(6.0, __dsqrt_rn(__ddiv_rn((double)thresh, (double)num_pair)));
    return (double)score < t;
}

__global__ __launch_bounds__(kThreads, 2) void gms_kernel(GmsArgs a) {
    __shared__ unsigned s_wh[kWaves][kMaxRight];   // per wave: right-cell histogram of the row in work (all zero between rows)
    __shared__ int s_hist[kCells], s_off[kCells + 1], s_cur[kCells], s_partner[kCells], s_acc[kCells];
    __shared__ int s_cnt[8], s_dev, s_wsum[kWaves];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const mlpl_dmatch *ml = a.matches + (size_t)b * a.match_stride;
    mlpl_dmatch *ol = a.out ? a.out + (size_t)b * a.match_stride : nullptr;
    int n = a.n_matches ? a.n_matches[b] : a.n_direct;
    n = min(max(n, 0), a.match_stride);
    int16_t *codes = a.codes + (size_t)b * 9 * a.S;
    uint16_t *bucket = a.bucket + (size_t)b * a.S;
    uint8_t *drop = a.drop + (size_t)b * a.S, *flags = a.flags + (size_t)b * a.S, *keep = a.keep + (size_t)b * a.S;

    // ---- cell codes (indices outside the keypoint arrays are clamped, never followed)
    for (int i = tid; i < n; i += kThreads) {
        const int q = min(max(ml[i].queryIdx, 0), a.nq - 1), t = min(max(ml[i].trainIdx, 0), a.nt - 1);
        const float2 p = reinterpret_cast<const float2 *>(a.kp1)[(size_t)b * a.nq + q], r = reinterpret_cast<const float2 *>(a.kp2)[(size_t)b * a.nt + t];
        const float xn = __fmul_rn(p.x, a.winv1), yn = __fmul_rn(p.y, a.hinv1);
        const float fx = __fmul_rn(xn, (float)kGrid), fy = __fmul_rn(yn, (float)kGrid);
        const float hx = __fadd_rn(fx, 0.5f), hy = __fadd_rn(fy, 0.5f);
        codes[0 * a.S + i] = (int16_t)left_code(fx, fy);
        codes[1 * a.S + i] = (int16_t)left_code(hx, fy);
        codes[2 * a.S + i] = (int16_t)left_code(fx, hy);
        codes[3 * a.S + i] = (int16_t)left_code(hx, hy);
        const float xr = __fmul_rn(r.x, a.winv2), yr = __fmul_rn(r.y, a.hinv2);
        for (int s = 0; s < a.n_scales; ++s) codes[(4 + s) * a.S + i] = (int16_t)right_code(xr, yr, kRightSize[s]);
        keep[i] = 0;
    }
    for (int i = tid; i < kWaves * kMaxRight; i += kThreads) (&s_wh[0][0])[i] = 0;
    __syncthreads();

    int best = 0, best_scale = -1, best_rot = -1, best_dev = 0;
    for (int s = 0; s < a.n_scales; ++s) {
        const int W = kRightSize[s];
        const int16_t *rc = codes + (size_t)(4 + s) * a.S;
        for (int i = tid; i < n; i += kThreads) drop[i] = 0, flags[i] = 0;
        if (tid == 0) s_dev = 0;
        for (int g = 0; g < 4; ++g) {
            const int16_t *lc = codes + (size_t)g * a.S;
            for (int i = tid; i < kCells; i += kThreads) s_hist[i] = 0;
            __syncthreads();
            // ---- assignMatchPairs: a match dropped here stays dropped for the later grid types of the run (the carried-over right index)
            for (int i = tid; i < n; i += kThreads) {
                if (drop[i]) continue;
                const int l = lc[i], r = rc[i];
                if (l < 0 || r < 0) {
                    drop[i] = 1;
                    if (l == kCodeDevDrop || r == kCodeDevDrop) atomicAdd(&s_dev, 1);
                } else {
                    atomicAdd(&s_hist[l], 1);
                }
            }
            __syncthreads();
            if (wave == 0) {   // exclusive scan of the 400 counts: 7 per lane
                int v[7], sum = 0;
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const int c = lane * 7 + k;
                    v[k] = c < kCells ? s_hist[c] : 0;
                    sum += v[k];
                }
                int inc = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int t = __shfl_up(inc, off);
                    if (lane >= off) inc += t;
                }
                int run = inc - sum;
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const int c = lane * 7 + k;
                    if (c < kCells) s_off[c] = run, s_cur[c] = run;
                    run += v[k];
                }
                if (lane == 63) s_off[kCells] = inc;
            }
            __syncthreads();
            for (int i = tid; i < n; i += kThreads) {
                if (drop[i]) continue;
                const int pos = atomicAdd(&s_cur[lc[i]], 1);
                bucket[pos] = (uint16_t)rc[i];
            }
            __syncthreads();
            // ---- verifyCellPairs: one wave per left cell
            unsigned *wh = s_wh[wave];
            for (int cell = wave; cell < kCells; cell += kWaves) {
                const int beg = s_off[cell], k = s_off[cell + 1] - beg;
                if (k == 0) {
                    if (lane == 0) s_partner[cell] = -1, s_acc[cell] = 0;
                    continue;
                }
                for (int e = lane; e < k; e += 64) atomicAdd(&wh[bucket[beg + e]], 1u);
                wave_sync();
                unsigned key = 0;   // (count, lowest right cell): the first maximum of the row
                for (int e = lane; e < k; e += 64) {
                    const unsigned v = bucket[beg + e];
                    key = max(key, (wh[v] << 16) | (0xFFFFu - v));
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, off));
                const int p = 0xFFFF - (int)(key & 0xFFFFu);
                wave_sync();
                for (int e = lane; e < k; e += 64) wh[bucket[beg + e]] = 0;
                wave_sync();
                // m[j] on lane kk = motion[left neighbour j][right neighbour kk of the partner]
                const int px = p % W, py = p / W, cx = cell % kGrid, cy = cell / kGrid;
                int m[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    m[j] = 0;
                    const int lx = cx + j % 3 - 1, ly = cy + j / 3 - 1;
                    if (lx < 0 || lx >= kGrid || ly < 0 || ly >= kGrid) continue;
                    const int ll = lx + kGrid * ly, b2 = s_off[ll], k2 = s_off[ll + 1] - b2;
                    for (int e0 = 0; e0 < k2; e0 += 64) {
                        int kk = -1;
                        if (e0 + lane < k2) {
                            const int v = bucket[b2 + e0 + lane], dx = v % W - px, dy = v / W - py;
                            if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) kk = dx + 1 + 3 * (dy + 1);
                        }
#pragma unroll
                        for (int q = 0; q < 9; ++q) {
                            const int c = __popcll(__ballot(kk == q));
                            if (lane == q) m[j] += c;
                        }
                    }
                }
                // lanes 0-7: rotation type = lane
                int score = 0, thresh = 0, num_pair = 0;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const int kk = j == 4 ? 4 : kRing[(kRingPos[j] - lane) & 7];
                    const int mv = __shfl(m[j], kk & 15);
                    const int lx = cx + j % 3 - 1, ly = cy + j / 3 - 1, rx = px + kk % 3 - 1, ry = py + kk / 3 - 1;
                    if (lx < 0 || lx >= kGrid || ly < 0 || ly >= kGrid || rx < 0 || rx >= W || ry < 0 || ry >= W) continue;
                    score += mv, thresh += s_hist[lx + kGrid * ly], ++num_pair;
                }
                const bool ok = lane < 8 && !gms_reject(score, thresh, num_pair);
                const unsigned long long okm = __ballot(ok);
                if (lane == 0) s_partner[cell] = p, s_acc[cell] = (int)(okm & 0xFFull) & a.rot_mask;
            }
            __syncthreads();
            // ---- mark: one inlier bit per rotation type, accumulated over the grid types
            for (int i = tid; i < n; i += kThreads) {
                if (drop[i]) continue;
                const int l = lc[i];
                if (s_partner[l] == rc[i]) flags[i] |= (uint8_t)s_acc[l];
            }
            __syncthreads();
        }
        // ---- the inlier counts of the scale level's runs; the first best run wins (strict >)
        if (tid < 8) s_cnt[tid] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += kThreads) {
            const int i = i0 + tid;
            const int f = i < n ? flags[i] : 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int c = __popcll(__ballot((f >> r) & 1));
                if (lane == 0 && c) atomicAdd(&s_cnt[r], c);
            }
        }
        __syncthreads();
        int win = -1;
        for (int r = 0; r < 8; ++r)
            if ((a.rot_mask >> r) & 1)
                if (s_cnt[r] > best) best = s_cnt[r], win = r;
        if (win >= 0) {
            best_scale = s, best_rot = win, best_dev = s_dev;
            for (int i = tid; i < n; i += kThreads) keep[i] = (flags[i] >> win) & 1;
        }
        __syncthreads();
    }

    // ---- result, the rule of correspondences.cpp:388-397 on request, ordered compaction
    const bool replace = a.rule ? best >= 2 : true;
    if (ol) {
        int base = 0;
        for (int c0 = 0; c0 < n; c0 += kThreads) {
            const int i = c0 + tid;
            const bool k = i < n && keep[i];
            const unsigned long long mask = __ballot(k);
            if (lane == 0) s_wsum[wave] = __popcll(mask);
            __syncthreads();
            int off = base, all = 0;
            for (int w = 0; w < kWaves; ++w) {
                if (w < wave) off += s_wsum[w];
                all += s_wsum[w];
            }
            off += __popcll(mask & ((1ull << lane) - 1ull));
            if (i < n) {
                if (!replace) ol[i] = ml[i];
                else if (k) ol[off] = ml[i];
            }
            base += all;
            __syncthreads();
        }
    }
    if (tid == 0) {
        int32_t *res = a.res + (size_t)b * 8;
        const int n_out = replace ? best : n;
        res[0] = best, res[1] = best_scale, res[2] = best_rot, res[3] = best_dev, res[4] = n_out, res[5] = 0, res[6] = 0, res[7] = 0;
        if (a.n_out) a.n_out[b] = n_out;
        if (a.n_inliers) a.n_inliers[b] = best;
    }
}

}  // namespace

int launch_gms(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, int n_direct,
               const float *d_kp1, int nq, const float *d_kp2, int nt, int width1, int height1, int width2, int height2, int use_scale,
               int use_rotation, int rule, mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_n_inliers, GmsWork *work, hipStream_t s) {
    const size_t S = ((size_t)std::max(match_stride, 1) + 63) / 64 * 64, B = (size_t)batch;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_codes = 0, o_bucket = o_codes + up(B * 9 * S * 2), o_drop = o_bucket + up(B * S * 2), o_flags = o_drop + up(B * S),
                 o_keep = o_flags + up(B * S), o_res = o_keep + up(B * S), total = o_res + up(B * 32);
    void *wsp = nullptr;
    int rc = ws_get(ctx, WS_GMS, total, &wsp);
    if (rc) return rc;
    char *w = static_cast<char *>(wsp);
    GmsArgs a{};
    a.matches = d_matches, a.n_matches = d_n_matches, a.kp1 = d_kp1, a.kp2 = d_kp2;
    a.match_stride = match_stride, a.nq = nq, a.nt = nt, a.n_direct = n_direct, a.n_scales = use_scale ? kScales : 1;
    a.rot_mask = use_rotation ? 0xFF : 1, a.rule = rule;
    // MatchGMS::normalizeKeypoints: the reciprocal first, in float
    a.winv1 = 1.0f / (float)width1, a.hinv1 = 1.0f / (float)height1, a.winv2 = 1.0f / (float)width2, a.hinv2 = 1.0f / (float)height2;
    a.S = S;
    a.codes = reinterpret_cast<int16_t *>(w + o_codes), a.bucket = reinterpret_cast<uint16_t *>(w + o_bucket);
    a.drop = reinterpret_cast<uint8_t *>(w + o_drop), a.flags = reinterpret_cast<uint8_t *>(w + o_flags);
    a.keep = reinterpret_cast<uint8_t *>(w + o_keep), a.res = reinterpret_cast<int32_t *>(w + o_res);
    a.out = d_out, a.n_out = d_n_out, a.n_inliers = d_n_inliers;
    hipLaunchKernelGGL(gms_kernel, dim3(batch), dim3(kThreads), 0, s, a);
    MLPL_HIP_TRY(hipGetLastError());
    if (work) work->keep = a.keep, work->res = a.res, work->stride = S;
    return MLPL_OK;
}

}  // namespace mlpl

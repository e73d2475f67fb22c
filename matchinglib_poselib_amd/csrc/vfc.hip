// vfc.hip -- the VFC match filter of matchinglib::getMatches (VFCrefine; M/source/vfcMatches.cpp:63-100 filterWithVFC, M/source/vfc.cpp: the
// default SparseVFC path, the only one the reference can reach) on gfx950.  One workgroup per problem, every EM iteration in one launch.
//
//   normalize()      vfc.cpp:560-621   bit for bit: the four means are strictly serial float sums, the scales serial double sums of exact
//                                      squares, both by single lanes over LDS-staged chunks; float divisions
//   selectSubset()   :130-150          one lane: `raw % n` of the 48 host-supplied rand() values, the 1e-3 L1 rejection on the float X
//   K, U, EM loop    :95-128, :152-188, :369-505   in float64 with the reference's float constants widened -- the m x m system is
//                                      numerically singular, so the device does not imitate the reference's float rounding
//
// Reductions: a wave owns the 64-point tiles wave, wave + 4, ...; per tile it stages U, Y and P in LDS, and 61 lanes own the 136 + 32
// accumulators of U diag(P) U^T and U diag(P) Y (three of one matrix row each), summing the tile's 64 terms in order.  Waves are added in
// order.  Every sum therefore has one fixed order that depends on n alone: a problem computes the same bits in any batch.
// Per-point state (X, Y, P, V and, with option "vfc_store_u", the 16 kernel values U) lives in the context workspace.
#include <algorithm>
#include <cfloat>
#include <vector>

#include "mlpl_internal.h"

namespace mlpl {

namespace {

constexpr int kThreads = 256, kWaves = 4, kCtrl = 16, kRows = 19, kPad = 65, kChunk = 1024;
constexpr int kRowYx = 16, kRowYy = 17, kRowP = 18;

struct VfcArgs {
    const mlpl_dmatch *matches;   // [batch][match_stride], or nullptr: the points come from x1 / x2
    const int32_t *n_matches;
    const float *kp1, *kp2;       // [batch][nq][2], [batch][nt][2]
    const float *x1, *x2;         // [n_direct][2] (single problem)
    const int32_t *raw;           // [batch][48] values of rand()
    int match_stride, nq, nt, n_direct, rule;
    size_t S;                     // workspace points per problem (a multiple of 64)
    float4 *pts;
    double *P, *U;
    double2 *V;
    uint8_t *keep;
    int32_t *res;                 // [batch][8] = {status, kept, m, iterations, refused, singular solves, n_out, 0}
    mlpl_dmatch *out;
    int32_t *n_out, *status;
};

__device__ __forceinline__ double rd_lane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the three sums over the workgroup, waves added in order; the same value in every thread
__device__ __forceinline__ void block_sum3(double &x, double &y, double &z, double (*s_w)[3]) {
    x = wave_sum(x), y = wave_sum(y), z = wave_sum(z);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[wave][0] = x, s_w[wave][1] = y, s_w[wave][2] = z;
    __syncthreads();
    x = s_w[0][0], y = s_w[0][1], z = s_w[0][2];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) x += s_w[w][0], y += s_w[w][1], z += s_w[w][2];
}

__device__ __forceinline__ double sq2(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}

template <bool kStoreU>
__global__ __launch_bounds__(kThreads, 2) void vfc_kernel(VfcArgs a) {
    __shared__ double s_rows[kWaves * kRows * kPad];   // per wave: U rows 0-15, Y.x, Y.y, P of its current tile; the float4 chunk of normalize()
    __shared__ double s_red[kWaves][64][3];
    __shared__ double s_A[kCtrl][kCtrl + 1], s_B[kCtrl][2], s_K[kCtrl][kCtrl + 1], s_C[kCtrl][2], s_tr[kCtrl], s_w[kWaves][3];
    __shared__ float s_cx[kCtrl], s_cy[kCtrl], s_f[8];
    __shared__ int s_int[8];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const mlpl_dmatch *ml = a.matches ? a.matches + (size_t)b * a.match_stride : nullptr;
    mlpl_dmatch *ol = a.out ? a.out + (size_t)b * a.match_stride : nullptr;
    int n = a.matches ? a.n_matches[b] : a.n_direct;
    n = min(max(n, 0), a.matches ? a.match_stride : a.n_direct);
    float4 *pts = a.pts + (size_t)b * a.S;
    double *Pw = a.P + (size_t)b * a.S;
    double2 *Vw = a.V + (size_t)b * a.S;
    double *Uw = kStoreU ? a.U + (size_t)b * a.S * kCtrl : nullptr;
    uint8_t *keep = a.keep + (size_t)b * a.S;
    int32_t *res = a.res + (size_t)b * 8;

    if (n < 5) {   // VFC::setData refuses (MIN_POINT_NUMBER): the list passes through
        for (int i = tid; i < n; i += kThreads) {
            keep[i] = 1, Pw[i] = 1.0;
            if (ol) ol[i] = ml[i];
        }
        if (tid == 0) {
            res[0] = -1, res[1] = n, res[2] = 0, res[3] = 0, res[4] = 0, res[5] = 0, res[6] = n, res[7] = 0;
            if (a.n_out) a.n_out[b] = n;
            if (a.status) a.status[b] = -1;
        }
        return;
    }

    // ---- the matched points (indices outside the keypoint arrays are clamped, never followed)
    for (int i = tid; i < n; i += kThreads) {
        float4 v;
        if (ml) {
            const int q = min(max(ml[i].queryIdx, 0), a.nq - 1), t = min(max(ml[i].trainIdx, 0), a.nt - 1);
            const float2 p = reinterpret_cast<const float2 *>(a.kp1)[(size_t)b * a.nq + q], r = reinterpret_cast<const float2 *>(a.kp2)[(size_t)b * a.nt + t];
            v = make_float4(p.x, p.y, r.x, r.y);
        } else {
            v = make_float4(a.x1[2 * i], a.x1[2 * i + 1], a.x2[2 * i], a.x2[2 * i + 1]);
        }
        pts[i] = v;
    }
    __syncthreads();

    // ---- normalize(): serial float means (lanes 0-3, one coordinate each) ...
    float4 *s_chunk = reinterpret_cast<float4 *>(s_rows);
    {
        float acc = 0.f;
        for (int c0 = 0; c0 < n; c0 += kChunk) {
            const int cn = min(kChunk, n - c0);
            for (int i = tid; i < cn; i += kThreads) s_chunk[i] = pts[c0 + i];
            __syncthreads();
            if (tid < 4) {
                const float *f = reinterpret_cast<const float *>(s_chunk) + tid;
                for (int k = 0; k < cn; ++k) acc += f[4 * k];
            }
            __syncthreads();
        }
        if (tid < 4) s_f[tid] = acc / (float)n;
        __syncthreads();
    }
    // ... then the centred points and the serial double sums of their squares (lane 0: left, lane 1: right)
    {
        const float mx1 = s_f[0], my1 = s_f[1], mx2 = s_f[2], my2 = s_f[3];
        double acc = 0.0;
        for (int c0 = 0; c0 < n; c0 += kChunk) {
            const int cn = min(kChunk, n - c0);
            for (int i = tid; i < cn; i += kThreads) {
                float4 v = pts[c0 + i];
                v.x -= mx1, v.y -= my1, v.z -= mx2, v.w -= my2;
                pts[c0 + i] = v, s_chunk[i] = v;
            }
            __syncthreads();
            if (tid < 2) {
                const float *f = reinterpret_cast<const float *>(s_chunk) + 2 * tid;
                for (int k = 0; k < cn; ++k) {
                    const double x = (double)f[4 * k], y = (double)f[4 * k + 1];
                    acc += x * x;
                    acc += y * y;
                }
            }
            __syncthreads();
        }
        if (tid < 2) s_f[4 + tid] = (float)sqrt(acc / (double)n);
        __syncthreads();
    }
    const float sc1 = s_f[4], sc2 = s_f[5];
    const bool refused = (double)sc1 < 0.1 || (double)sc2 < 0.1;   // MIN_STANDARD_DEVIATION: optimize() returns, every match is kept

    int m = 0, iters = 0, kept = n, singular = 0;
    const int ntile = (n + 63) >> 6, nround = (ntile + kWaves - 1) / kWaves;
    double *rows = s_rows + wave * kRows * kPad;

    if (!refused) {
        for (int i = tid; i < n; i += kThreads) {
            const float4 v = pts[i];
            const float lx = v.x / sc1, ly = v.y / sc1, rx = v.z / sc2, ry = v.w / sc2;
            pts[i] = make_float4(lx, ly, rx - lx, ry - ly);   // X, Y
        }
        __syncthreads();

        // ---- selectSubset()
        if (tid == 0) {
            const int want = min(kCtrl, n);
            const int32_t *raw = a.raw + (size_t)b * 3 * kCtrl;
            int cnt = 0;
            for (int it = 0; cnt < want && it < 3 * want; ++it) {
                const float4 v = pts[raw[it] % n];
                float dist = 1.0e30f;
                for (int c = 0; c < cnt; ++c) dist = fminf(fabsf(s_cx[c] - v.x) + fabsf(s_cy[c] - v.y), dist);
                if ((double)dist > 1e-3) s_cx[cnt] = v.x, s_cy[cnt] = v.y, ++cnt;
            }
            s_int[0] = cnt;
        }
        __syncthreads();
        m = s_int[0];

        const double beta = (double)0.1f, lam = 3.0, av = 10.0, ecr = (double)1e-5f, minP = (double)1e-5f, two_pi = (double)6.283185f,
                     theta = (double)0.75f;
        {
            const int i = tid >> 4, j = tid & 15;
            double k = 0.0;
            if (i < m && j < m) k = i == j ? 1.0 : exp(-beta * sq2((double)s_cx[i], (double)s_cy[i], (double)s_cx[j], (double)s_cy[j]));
            s_K[i][j] = k;
            if (tid < kCtrl) s_C[tid][0] = 0.0, s_C[tid][1] = 0.0;
        }
        __syncthreads();
        if (tid >= m && tid < kCtrl) s_cx[tid] = 0.f, s_cy[tid] = 0.f;   // (rows m .. 15 of U are zero; their exp is computed and dropped)
        __syncthreads();

        // which accumulators this lane owns: row la, columns lb .. lb + 2 of [U P U^T | U P Y] (columns 16, 17 = Y.x, Y.y)
        int la = 0, lb = 18;
        {
            int cnt = 0;
            for (int r = 0; r < kCtrl; ++r) {
                const int nl = (18 - r + 2) / 3;
                if (lane >= cnt && lane < cnt + nl) la = r, lb = r + 3 * (lane - cnt);
                cnt += nl;
            }
        }
        const int c0i = min(lb, 17), c1i = min(lb + 1, 17), c2i = min(lb + 2, 17);

        // ---- initialize(): V = 0, P = 1, sigma^2; U once when it is kept
        double s2 = 0.0, sp = 0.0, cntd = 0.0;
        for (int rr = 0; rr < nround; ++rr) {
            const int i = ((rr * kWaves + wave) << 6) + lane;
            if (i < n) {
                const float4 v = pts[i];
                Vw[i] = make_double2(0.0, 0.0);
                Pw[i] = 1.0;
                s2 += sq2((double)v.z, (double)v.w, 0.0, 0.0);
                sp += 1.0;
                if (kStoreU) {
#pragma unroll
                    for (int r = 0; r < kCtrl; ++r)
                        Uw[((size_t)(i >> 6) * kCtrl + r) * 64 + lane] = r < m ? exp(-beta * sq2((double)s_cx[r], (double)s_cy[r], (double)v.x, (double)v.y)) : 0.0;
                }
            }
        }
        block_sum3(s2, sp, cntd, s_w);
        double sigma2 = s2 / (sp * 2.0), gamma = (double)0.9f, E = 1.0, tecr = 1.0;

        while (iters < 50 && tecr > ecr && sigma2 > 1e-8) {
            const double E_old = E;
            // ---- getP() and the sums of calculateC_SparseVFC()
            const double temp2 = two_pi * sigma2 * (1.0 - gamma) / (gamma * av);
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, sumP = 0.0, sumE = 0.0, zero = 0.0;
            for (int rr = 0; rr < nround; ++rr) {
                const int tile = rr * kWaves + wave, i = (tile << 6) + lane;
                const bool valid = i < n;
                double p = 0.0, yx = 0.0, yy = 0.0;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                __syncthreads();   // the previous tile's readers are done
                if (valid) {
                    v = pts[i];
                    const double2 V = Vw[i];
                    yx = (double)v.z, yy = (double)v.w;
                    const double t = sq2(yx, yy, V.x, V.y);
                    const double temp1 = exp(-t / (2.0 * sigma2));
                    const double pp = temp1 / (temp1 + temp2);
                    p = fmax(minP, pp);
                    Pw[i] = p;
                    sumP += pp;
                    sumE += pp * t;
                }
#pragma unroll 4
                for (int r = 0; r < kCtrl; ++r) {
                    double u = 0.0;
                    if (valid) {
                        if (kStoreU) u = Uw[((size_t)tile * kCtrl + r) * 64 + lane];
                        else u = r < m ? exp(-beta * sq2((double)s_cx[r], (double)s_cy[r], (double)v.x, (double)v.y)) : 0.0;
                    }
                    rows[r * kPad + lane] = u;
                }
                rows[kRowYx * kPad + lane] = yx, rows[kRowYy * kPad + lane] = yy, rows[kRowP * kPad + lane] = p;
                __syncthreads();
                if (tile < ntile) {
                    const double *ra = rows + la * kPad, *r0 = rows + c0i * kPad, *r1 = rows + c1i * kPad, *r2 = rows + c2i * kPad,
                                 *rp = rows + kRowP * kPad;
#pragma unroll 8
                    for (int k = 0; k < 64; ++k) {
                        const double l = rp[k] * ra[k];
                        acc0 += l * r0[k];
                        acc1 += l * r1[k];
                        acc2 += l * r2[k];
                    }
                }
            }
            s_red[wave][lane][0] = acc0, s_red[wave][lane][1] = acc1, s_red[wave][lane][2] = acc2;
            block_sum3(sumP, sumE, zero, s_w);   // (its barriers also publish s_red)
            if (tid < 64) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int c = lb + j;
                    if (c > 17) continue;
                    double tot = s_red[0][tid][j];
#pragma unroll
                    for (int w = 1; w < kWaves; ++w) tot += s_red[w][tid][j];
                    if (c < kCtrl) {
                        tot += lam * sigma2 * s_K[la][c];
                        s_A[la][c] = tot, s_A[c][la] = tot;
                    } else {
                        s_B[la][c - kCtrl] = tot;
                    }
                }
                // calculateTraceCKC() on the previous C
                if (tid < kCtrl) {
                    double kx = 0.0, ky = 0.0;
                    for (int j = 0; j < m; ++j) kx += s_K[tid][j] * s_C[j][0], ky += s_K[tid][j] * s_C[j][1];
                    s_tr[tid] = s_C[tid][0] * kx + s_C[tid][1] * ky;
                }
            }
            __syncthreads();
            {
                double trace = 0.0;
                for (int i = 0; i < m; ++i) trace += s_tr[i];
                E = sumE / (2.0 * sigma2) + sumP * log(sigma2);
                E += lam / 2.0 * trace;
                tecr = fabs((E - E_old) / E);
            }
            // ---- cv::solve(DECOMP_LU) on the m x m system: lane j of wave 0 holds row j of [A | B]
            if (tid < 64) {
                double r[18];
                const int row = min(lane, kCtrl - 1);
#pragma unroll
                for (int k = 0; k < kCtrl; ++k) r[k] = s_A[row][k];
                r[16] = s_B[row][0], r[17] = s_B[row][1];
                bool sing = false;
#pragma unroll
                for (int i = 0; i < kCtrl; ++i) {
                    if (i < m && !sing) {
                        int p = i;
                        double best = fabs(rd_lane(r[i], i));
#pragma unroll
                        for (int j = i + 1; j < kCtrl; ++j) {
                            const double v = fabs(rd_lane(r[i], j));
                            if (j < m && v > best) best = v, p = j;
                        }
                        if (best < 100.0 * DBL_EPSILON) {
                            sing = true;
                        } else {
                            p = __builtin_amdgcn_readfirstlane(p);
                            if (p != i) {
#pragma unroll
                                for (int k = i; k < 18; ++k) {
                                    const double vi = rd_lane(r[k], i), vp = rd_lane(r[k], p);
                                    r[k] = lane == i ? vp : (lane == p ? vi : r[k]);
                                }
                            }
                            const double d = -1.0 / rd_lane(r[i], i);
                            const double alpha = r[i] * d;
                            const bool below = lane > i && lane < m;
#pragma unroll
                            for (int k = i + 1; k < 18; ++k) {
                                const double pv = rd_lane(r[k], i);
                                if (below) r[k] += alpha * pv;
                            }
                            if (lane == i) r[i] = -d;
                        }
                    }
                }
                double x0[kCtrl], x1[kCtrl], c0 = 0.0, c1 = 0.0;
#pragma unroll
                for (int i = kCtrl - 1; i >= 0; --i) {
                    x0[i] = 0.0, x1[i] = 0.0;
                    if (i < m && !sing) {
                        double s0 = r[16], s1 = r[17];
#pragma unroll
                        for (int k = i + 1; k < kCtrl; ++k) {
                            if (k < m) s0 -= r[k] * x0[k], s1 -= r[k] * x1[k];
                        }
                        s0 *= r[i], s1 *= r[i];
                        if (lane == i) c0 = s0, c1 = s1;
                        x0[i] = rd_lane(s0, i), x1[i] = rd_lane(s1, i);
                    }
                }
                if (lane < kCtrl) s_C[lane][0] = c0, s_C[lane][1] = c1;
                if (lane == 0) s_int[1] = sing ? 1 : 0;
            }
            __syncthreads();
            singular += s_int[1];
            // ---- calculateV(), calculateSigmaSquare(), calculateGamma()
            s2 = 0.0, sp = 0.0, cntd = 0.0;
            for (int rr = 0; rr < nround; ++rr) {
                const int tile = rr * kWaves + wave, i = (tile << 6) + lane;
                if (i < n) {
                    const float4 v = pts[i];
                    double vx = 0.0, vy = 0.0;
#pragma unroll 4
                    for (int r = 0; r < kCtrl; ++r) {
                        double u;
                        if (kStoreU) u = Uw[((size_t)tile * kCtrl + r) * 64 + lane];
                        else u = r < m ? exp(-beta * sq2((double)s_cx[r], (double)s_cy[r], (double)v.x, (double)v.y)) : 0.0;
                        vx += u * s_C[r][0], vy += u * s_C[r][1];
                    }
                    Vw[i] = make_double2(vx, vy);
                    const double p = Pw[i];
                    s2 += p * sq2((double)v.z, (double)v.w, vx, vy);
                    sp += p;
                    cntd += p > theta ? 1.0 : 0.0;
                }
            }
            block_sum3(s2, sp, cntd, s_w);
            sigma2 = s2 / (sp * 2.0);
            kept = (int)cntd;
            gamma = fmax(fmin(cntd / (double)n, (double)0.95f), (double)0.05f);
            ++iters;
        }
    }

    // ---- filterWithVFC's result, getMatches' replacement rule (matchers.cpp:726-731), ordered compaction
    const double theta = (double)0.75f;
    const int status = (double)kept / (double)n < 0.1 ? -2 : 0;
    const bool replace = a.rule ? (status == 0 && (kept > 8 || n < 24)) : true;
    int base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += kThreads) {
        const int i = c0 + tid;
        bool k = false;
        if (i < n) {
            if (iters > 0) k = Pw[i] > theta;
            else k = true, Pw[i] = 1.0;
            keep[i] = k ? 1 : 0;
        }
        if (ol) {
            const unsigned long long mask = __ballot(k);
            if (lane == 0) s_int[4 + wave] = __popcll(mask);
            __syncthreads();
            int off = base;
            for (int w = 0; w < wave; ++w) off += s_int[4 + w];
            off += __popcll(mask & ((1ull << lane) - 1ull));
            if (i < n) {
                if (!replace) ol[i] = ml[i];
                else if (k) ol[off] = ml[i];
            }
            base += s_int[4] + s_int[5] + s_int[6] + s_int[7];
            __syncthreads();
        }
    }
    if (tid == 0) {
        const int n_out = replace ? kept : n;
        res[0] = status, res[1] = kept, res[2] = m, res[3] = iters, res[4] = refused ? 1 : 0, res[5] = singular, res[6] = n_out, res[7] = 0;
        if (a.n_out) a.n_out[b] = n_out;
        if (a.status) a.status[b] = status;
    }
}

thread_local std::vector<int32_t> t_raw;   // grows monotonically: no allocation on the steady path

}  // namespace

int launch_vfc(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, const float *d_kp1, int nq,
               const float *d_kp2, int nt, const float *d_x1, const float *d_x2, int n_direct, const uint32_t *seeds, int rule, mlpl_dmatch *d_out,
               int32_t *d_n_out, int32_t *d_status, VfcWork *work, hipStream_t s) {
    const int limit = d_matches ? match_stride : n_direct;
    const size_t S = ((size_t)std::max(limit, 1) + 63) / 64 * 64, B = (size_t)batch;
    const bool store_u = ctx->opt_vfc_store_u != 0;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_pts = 0, o_P = o_pts + up(B * S * 16), o_V = o_P + up(B * S * 8), o_keep = o_V + up(B * S * 16), o_res = o_keep + up(B * S),
                 o_raw = o_res + up(B * 32), o_U = o_raw + up(B * 3 * kCtrl * 4), total = o_U + (store_u ? up(B * S * kCtrl * 8) : 0);
    void *wsp = nullptr;
    int rc = ws_get(ctx, WS_VFC, total, &wsp);
    if (rc) return rc;
    char *w = static_cast<char *>(wsp);
    // the raw rand() values of every problem's seed (glibc; the device reduces them modulo ITS n)
    if (t_raw.size() < B * 3 * kCtrl) t_raw.resize(B * 3 * kCtrl);
    GlibcRand gen;
    for (size_t b = 0; b < B; ++b) {
        if (b > 0 && seeds && seeds[b] == seeds[b - 1]) {
            std::copy(t_raw.begin() + (b - 1) * 3 * kCtrl, t_raw.begin() + b * 3 * kCtrl, t_raw.begin() + b * 3 * kCtrl);
            continue;
        }
        gen.seed(seeds ? seeds[b] : 1u);
        for (int k = 0; k < 3 * kCtrl; ++k) t_raw[b * 3 * kCtrl + k] = gen.next();
        if (!seeds) {
            for (size_t c = 1; c < B; ++c) std::copy(t_raw.begin(), t_raw.begin() + 3 * kCtrl, t_raw.begin() + c * 3 * kCtrl);
            break;
        }
    }
    // t_raw is pageable and reused by this thread's next call: that is safe because an asynchronous copy FROM pageable host memory has consumed
    // its source when it returns, at any size (up to 65535 x 192 bytes here) -- the runtime stages it, or pins it and waits; only the device
    // side is stream-ordered.  (linear_refine_impl.h relies on the same rule.)
    MLPL_HIP_TRY(hipMemcpyAsync(w + o_raw, t_raw.data(), B * 3 * kCtrl * 4, hipMemcpyHostToDevice, s));
    VfcArgs a{};
    a.matches = d_matches, a.n_matches = d_n_matches, a.kp1 = d_kp1, a.kp2 = d_kp2, a.x1 = d_x1, a.x2 = d_x2;
    a.raw = reinterpret_cast<const int32_t *>(w + o_raw);
    a.match_stride = match_stride, a.nq = nq, a.nt = nt, a.n_direct = n_direct, a.rule = rule, a.S = S;
    a.pts = reinterpret_cast<float4 *>(w + o_pts), a.P = reinterpret_cast<double *>(w + o_P), a.V = reinterpret_cast<double2 *>(w + o_V);
    a.U = store_u ? reinterpret_cast<double *>(w + o_U) : nullptr;
    a.keep = reinterpret_cast<uint8_t *>(w + o_keep), a.res = reinterpret_cast<int32_t *>(w + o_res);
    a.out = d_out, a.n_out = d_n_out, a.status = d_status;
    if (store_u) hipLaunchKernelGGL(vfc_kernel<true>, dim3(batch), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(vfc_kernel<false>, dim3(batch), dim3(kThreads), 0, s, a);
    MLPL_HIP_TRY(hipGetLastError());
    if (work) work->keep = a.keep, work->P = a.P, work->res = a.res, work->stride = S;
    return MLPL_OK;
}

}  // namespace mlpl

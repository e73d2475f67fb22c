// rectify.hip -- stereo rectification: poselib::getRectificationParameters with globRectFunct = true (rectifyFusiello,
// P/source/pose_helper.cpp:1366-1857, with cvUndistortPoints2 :2290-2412 and icvGetRectanglesV0 :2429-2503), cv::initUndistortRectifyMap
// (CV_32FC1) and the cv::remap(INTER_LINEAR, BORDER_CONSTANT) of poselib::GetRectifiedImages (:2775-2793).
// The contract, the operation order and the declared deviations: include/mlpl_c.h; the order itself is written down once, in
// tests/rectify_oracle.py, and everything here follows it line by line (the build has -ffp-contract=off on host and device).
//
// The parameters are host arithmetic on a handful of 3 x 3 matrices and need no device.  Three kernels: rectify_maps_kernel (the maps),
// remap_kernel (a remap through maps in memory) and rectify_fused_kernel (the hot path: a batch of pairs, the image index is grid.z, every
// lane computes the map values of 4 adjacent output pixels in registers, rounds them to float32 as the map kernel does, samples and stores
// the 4 bytes with one store; no map reaches memory).  All three share map_pixel / remap_pixel, so the fused result is the two-step one.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "mlpl_internal.h"

namespace mlpl {

namespace {

// ---------------------------------------------------------------------------------------------------------------- host: the parameters
void mul3(const double *a, const double *b, double *c) {
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = a[3 * i] * b[j];
            s = s + a[3 * i + 1] * b[3 + j];
            s = s + a[3 * i + 2] * b[6 + j];
            r[3 * i + j] = s;
        }
    for (int i = 0; i < 9; ++i) c[i] = r[i];
}

void mulv3(const double *a, const double *v, double *out) {
    double r[3];
    for (int i = 0; i < 3; ++i) {
        double s = a[3 * i] * v[0];
        s = s + a[3 * i + 1] * v[1];
        s = s + a[3 * i + 2] * v[2];
        r[i] = s;
    }
    out[0] = r[0], out[1] = r[1], out[2] = r[2];
}

// adjugate over determinant, the determinant expanded along the first row
void inv3(const double *m, double *o) {
    const double c00 = m[4] * m[8] - m[5] * m[7];
    const double c01 = m[5] * m[6] - m[3] * m[8];
    const double c02 = m[3] * m[7] - m[4] * m[6];
    double det = m[0] * c00;
    det = det + m[1] * c01;
    det = det + m[2] * c02;
    const double d = 1.0 / det;
    double r[9] = {c00 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
                   c01 * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                   c02 * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d};
    for (int i = 0; i < 9; ++i) o[i] = r[i];
}

struct P2f {
    float x, y;
};

// cvUndistortPoints2 in place on n float points; k == nullptr: no coefficients (one pass); RR == nullptr: identity
void undistort_points(P2f *pts, int n, const double *A, const double *k, const double *RR, bool *mask) {
    static const double zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int iters = k ? 5 : 1;
    if (!k) k = zero;
    const double fx = A[0], fy = A[4], cx = A[2], cy = A[5];
    const double ifx = 1.0 / fx, ify = 1.0 / fy;
    for (int i = 0; i < n; ++i) {
        double x = ((double)pts[i].x - cx) * ifx, y = ((double)pts[i].y - cy) * ify;
        const double x0 = x, y0 = y;
        for (int j = 0; j < iters; ++j) {
            const double r2 = x * x + y * y;
            const double icdist = (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            const double dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x);
            const double dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
        {
            const double r2 = x * x + y * y;
            const double icdist = (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2);
            const double dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x);
            const double dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y;
            const float qx = (float)(x * icdist + dx - x0), qy = (float)(y * icdist + dy - y0);   // Point2f proofdist
            const float qxx = qx * qx, qyy = qy * qy;
            const float d = std::sqrt(qxx + qyy);
            mask[i] = !((double)d > 0.25);   // a NaN passes, as in the reference
        }
        if (RR) {
            const double xx = RR[0] * x + RR[1] * y + RR[2];
            const double yy = RR[3] * x + RR[4] * y + RR[5];
            const double ww = 1.0 / (RR[6] * x + RR[7] * y + RR[8]);
            x = xx * ww;
            y = yy * ww;
        }
        pts[i].x = (float)x, pts[i].y = (float)y;
    }
}

// rectifyFusiello :1703-1744
int corner_points(const double *A, const double *k, double nx, double ny, P2f *pts) {
    P2f sv[4];
    bool mask[4];
    for (int i = 0; i < 4; ++i) {
        const int j = i < 2 ? 0 : 1;
        pts[i].x = (float)((i % 2) * (nx - 1.0));
        pts[i].y = (float)(j * (ny - 1.0));
        sv[i] = pts[i];
    }
    double reduction = 0.01;
    int steps = 0, valid;
    const double cx = nx / 2.0, cy = ny / 2.0;
    do {
        undistort_points(pts, 4, A, k, nullptr, mask);
        valid = 0;
        for (int i = 0; i < 4; ++i) valid += mask[i] ? 1 : 0;
        if (valid < 4) {
            for (int i = 0; i < 4; ++i) {
                const int j = i < 2 ? 0 : 1;
                if (!mask[i]) {
                    sv[i].x = pts[i].x = (float)(std::floor((1.0 - reduction) * ((i % 2) * nx - cx)) + cx - 1.0);
                    sv[i].y = pts[i].y = (float)(std::floor((1.0 - reduction) * (j * ny - cy)) + cy - 1.0);
                } else {
                    pts[i] = sv[i];
                }
            }
            reduction = reduction + 0.01;
            ++steps;
        }
    } while (valid < 4 && reduction < 0.25);
    if (reduction >= 0.25) undistort_points(pts, 4, A, nullptr, nullptr, mask);
    return steps;
}

struct Rectf {
    float x, y, width, height;
};

// icvGetRectanglesV0 on the 9 x 9 grid
int rectangles(const double *A, const double *k, const double *Rk, const double *pp, int w, int h, Rectf *inner, Rectf *outer) {
    constexpr int N = 9;
    double RR[9];
    mul3(pp, Rk, RR);
    P2f grid[N * N], pts[N * N], sv[N * N];
    bool mask[N * N];
    for (int y = 0, q = 0; y < N; ++y)
        for (int x = 0; x < N; ++x, ++q) {
            const float gx = (float)x * (float)w, gy = (float)y * (float)h;
            grid[q].x = gx / (float)(N - 1), grid[q].y = gy / (float)(N - 1);
            pts[q] = sv[q] = grid[q];
        }
    float reduction = 0.01f;
    int steps = 0, valid;
    const float cx = (float)w / 2.f, cy = (float)h / 2.f;
    do {
        undistort_points(pts, N * N, A, k, RR, mask);
        valid = 0;
        for (int i = 0; i < N * N; ++i) valid += mask[i] ? 1 : 0;
        if (valid < N * N) {
            const double red = 1.0 - (double)reduction;
            for (int i = 0; i < N * N; ++i) {
                if (!mask[i]) {
                    const float ex = grid[i].x - cx, ey = grid[i].y - cy;
                    sv[i].x = pts[i].x = (float)(red * (double)ex + (double)cx);
                    sv[i].y = pts[i].y = (float)(red * (double)ey + (double)cy);
                } else {
                    pts[i] = sv[i];
                }
            }
            reduction = reduction + 0.01f;
            ++steps;
        }
    } while (valid < N * N && (double)reduction < 0.25);
    if ((double)reduction >= 0.25) undistort_points(pts, N * N, A, nullptr, RR, mask);
    float iX0 = -FLT_MAX, iX1 = FLT_MAX, iY0 = -FLT_MAX, iY1 = FLT_MAX;
    float oX0 = FLT_MAX, oX1 = -FLT_MAX, oY0 = FLT_MAX, oY1 = -FLT_MAX;
    for (int y = 0, q = 0; y < N; ++y)
        for (int x = 0; x < N; ++x, ++q) {
            const P2f p = pts[q];
            oX0 = std::min(oX0, p.x), oX1 = std::max(oX1, p.x), oY0 = std::min(oY0, p.y), oY1 = std::max(oY1, p.y);
            if (x == 0) iX0 = std::max(iX0, p.x);
            if (x == N - 1) iX1 = std::min(iX1, p.x);
            if (y == 0) iY0 = std::max(iY0, p.y);
            if (y == N - 1) iY1 = std::min(iY1, p.y);
        }
    *inner = Rectf{iX0, iY0, iX1 - iX0, iY1 - iY0};
    *outer = Rectf{oX0, oY0, oX1 - oX0, oY1 - oY0};
    return steps;
}

// (int) of a double: NaN -> 0, saturating (the reference's cast is undefined there)
long long sat_int(double x) {
    if (x != x) return 0;
    return (long long)std::max(-2147483648.0, std::min(2147483647.0, x));
}

bool finite_all(const double *p, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- device
struct MapParams {
    double ir[9];    // (Knew Rect)^-1
    double k[8];     // k1, k2, p1, p2, k3, k4, k5, k6
    double fx, fy, cx, cy;
};

// {K[9], dist[8], Rect[9], Knew[9]} -> MapParams; false when a value is not finite
bool make_map_params(const double *K, const double *dist, int n_dist, const double *Rect, const double *Knew, MapParams *p) {
    if (!finite_all(K, 9) || !finite_all(Rect, 9) || !finite_all(Knew, 9) || (n_dist > 0 && !finite_all(dist, n_dist))) return false;
    double A[9];
    mul3(Knew, Rect, A);
    inv3(A, p->ir);
    for (int i = 0; i < 8; ++i) p->k[i] = i < n_dist ? dist[i] : 0.0;
    p->fx = K[0], p->fy = K[4], p->cx = K[2], p->cy = K[5];
    return true;
}

constexpr int kPix = 4;           // adjacent pixels per lane
constexpr int kLanesX = 64, kRows = 4;
constexpr int kMaxSide = 16384;

__device__ inline void map_pixel(const MapParams &p, int ui, int vi, float *mx, float *my) {
    const double u = (double)ui, v = (double)vi;
    double _x = v * p.ir[1];
    _x = _x + p.ir[2];
    _x = u * p.ir[0] + _x;
    double _y = v * p.ir[4];
    _y = _y + p.ir[5];
    _y = u * p.ir[3] + _y;
    double _w = v * p.ir[7];
    _w = _w + p.ir[8];
    _w = u * p.ir[6] + _w;
    const double x = _x / _w;
    const double y = _y / _w;
    const double x2 = x * x;
    const double y2 = y * y;
    const double r2 = x2 + y2;
    const double _2xy = (2.0 * x) * y;
    double num = p.k[4] * r2;
    num = num + p.k[1];
    num = num * r2;
    num = num + p.k[0];
    num = num * r2;
    num = 1.0 + num;
    double den = p.k[7] * r2;
    den = den + p.k[6];
    den = den * r2;
    den = den + p.k[5];
    den = den * r2;
    den = 1.0 + den;
    const double kr = num / den;
    double xd = x * kr;
    xd = xd + p.k[2] * _2xy;
    xd = xd + p.k[3] * (r2 + 2.0 * x2);
    double yd = y * kr;
    yd = yd + p.k[2] * (r2 + 2.0 * y2);
    yd = yd + p.k[3] * _2xy;
    *mx = (float)(p.fx * xd + p.cx);
    *my = (float)(p.fy * yd + p.cy);
}

__device__ inline bool fits_int(float x) { return x >= -2147483648.0f && x < 2147483648.0f; }   // false for NaN

__device__ inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// OpenCV's fixed-point bilinear tap sum; a tap outside the image adds nothing
__device__ inline uint32_t remap_pixel(const uint8_t *img, size_t step, int w, int h, float mx, float my) {
    const float ax = mx * 32.f, ay = my * 32.f;
    if (!(fits_int(ax) && fits_int(ay))) return 0u;      // NaN, or the rounding would not fit an int: outside
    const int sx = (int)rintf(ax), sy = (int)rintf(ay);  // round half even
    const int ix = sat16(sx >> 5), iy = sat16(sy >> 5);
    const int fx = sx & 31, fy = sy & 31;
    const bool x0 = ix >= 0 && ix < w, x1 = ix + 1 >= 0 && ix + 1 < w;
    const bool y0 = iy >= 0 && iy < h, y1 = iy + 1 >= 0 && iy + 1 < h;
    int acc = 0;
    // No source address is formed before the tap has passed the inside test: the row pointer only under y0 / y1, the column offset only
    // under x0 / x1.  A hostile map value therefore never reaches an address.
    if (y0) {
        const uint8_t *row = img + (size_t)iy * step;
        if (x0) acc += (32 - fx) * (32 - fy) * 32 * (int)row[ix];
        if (x1) acc += fx * (32 - fy) * 32 * (int)row[ix + 1];
    }
    if (y1) {
        const uint8_t *row = img + (size_t)(iy + 1) * step;
        if (x0) acc += (32 - fx) * fy * 32 * (int)row[ix];
        if (x1) acc += fx * fy * 32 * (int)row[ix + 1];
    }
    return (uint32_t)((acc + 16384) >> 15);
}

__global__ __launch_bounds__(kLanesX *kRows) void rectify_maps_kernel(MapParams p, int width, int height, float *mapx, float *mapy, size_t stride,
                                                                      int vec_ok) {
    const int x0 = ((int)blockIdx.x * kLanesX + (int)threadIdx.x) * kPix, y = (int)blockIdx.y * kRows + (int)threadIdx.y;
    if (x0 >= width || y >= height) return;
    float mx[kPix], my[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) map_pixel(p, x0 + i, y, &mx[i], &my[i]);
    float *rx = mapx + (size_t)y * stride + x0, *ry = mapy + (size_t)y * stride + x0;
    if (vec_ok && x0 + kPix <= width) {
        *reinterpret_cast<float4 *>(rx) = make_float4(mx[0], mx[1], mx[2], mx[3]);
        *reinterpret_cast<float4 *>(ry) = make_float4(my[0], my[1], my[2], my[3]);
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (x0 + i < width) rx[i] = mx[i], ry[i] = my[i];
    }
}

__device__ inline void store_pixels(uint8_t *row, int x0, int width, const uint32_t v[kPix], int vec_ok) {
    if (vec_ok && x0 + kPix <= width) {
        *reinterpret_cast<uint32_t *>(row + x0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (x0 + i < width) row[x0 + i] = (uint8_t)v[i];
    }
}

__global__ __launch_bounds__(kLanesX *kRows) void remap_kernel(const uint8_t *img, int width, int height, size_t step, const float *mapx,
                                                               const float *mapy, size_t stride, int map_vec_ok, int out_width, int out_height,
                                                               uint8_t *out, size_t out_step, int out_vec_ok) {
    const int x0 = ((int)blockIdx.x * kLanesX + (int)threadIdx.x) * kPix, y = (int)blockIdx.y * kRows + (int)threadIdx.y;
    if (x0 >= out_width || y >= out_height) return;
    const float *rx = mapx + (size_t)y * stride + x0, *ry = mapy + (size_t)y * stride + x0;
    float mx[kPix] = {0.f, 0.f, 0.f, 0.f}, my[kPix] = {0.f, 0.f, 0.f, 0.f};
    if (map_vec_ok && x0 + kPix <= out_width) {
        const float4 a = *reinterpret_cast<const float4 *>(rx), b = *reinterpret_cast<const float4 *>(ry);
        mx[0] = a.x, mx[1] = a.y, mx[2] = a.z, mx[3] = a.w, my[0] = b.x, my[1] = b.y, my[2] = b.z, my[3] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (x0 + i < out_width) mx[i] = rx[i], my[i] = ry[i];
    }
    uint32_t v[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) v[i] = x0 + i < out_width ? remap_pixel(img, step, width, height, mx[i], my[i]) : 0u;
    store_pixels(out + (size_t)y * out_step, x0, out_width, v, out_vec_ok);
}

struct FusedArgs {
    const uint8_t *img[2];
    uint8_t *out[2];
    const MapParams *params;   // [batch][2]
    size_t step, batch_stride, out_step, out_batch_stride;
    int width, height, out_width, out_height, out_vec_ok;
};

__global__ __launch_bounds__(kLanesX *kRows) void rectify_fused_kernel(FusedArgs a) {
    const int x0 = ((int)blockIdx.x * kLanesX + (int)threadIdx.x) * kPix, y = (int)blockIdx.y * kRows + (int)threadIdx.y;
    if (x0 >= a.out_width || y >= a.out_height) return;
    const int image = (int)blockIdx.z, b = image >> 1, side = image & 1;
    const MapParams &p = a.params[image];
    const uint8_t *img = a.img[side] + (size_t)b * a.batch_stride;
    uint32_t v[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
        float mx, my;
        map_pixel(p, x0 + i, y, &mx, &my);   // rounded to float32 as the map kernel stores them
        v[i] = x0 + i < a.out_width ? remap_pixel(img, a.step, a.width, a.height, mx, my) : 0u;
    }
    store_pixels(a.out[side] + (size_t)b * a.out_batch_stride + (size_t)y * a.out_step, x0, a.out_width, v, a.out_vec_ok);
}

dim3 grid_for(int width, int height, int images) {
    return dim3((width + kLanesX * kPix - 1) / (kLanesX * kPix), (height + kRows - 1) / kRows, images);
}

int launch_maps(const MapParams &p, int width, int height, float *d_mapx, float *d_mapy, size_t stride, hipStream_t s) {
    const int vec_ok = stride % 4 == 0 && (uintptr_t)d_mapx % 16 == 0 && (uintptr_t)d_mapy % 16 == 0;
    hipLaunchKernelGGL(rectify_maps_kernel, grid_for(width, height, 1), dim3(kLanesX, kRows), 0, s, p, width, height, d_mapx, d_mapy, stride, vec_ok);
    MLPL_HIP_TRY(hipGetLastError());
    return MLPL_OK;
}

int launch_remap(const uint8_t *d_img, int width, int height, size_t step, const float *d_mapx, const float *d_mapy, size_t stride,
                 int out_width, int out_height, uint8_t *d_out, size_t out_step, hipStream_t s) {
    const int map_vec_ok = stride % 4 == 0 && (uintptr_t)d_mapx % 16 == 0 && (uintptr_t)d_mapy % 16 == 0;
    const int out_vec_ok = out_step % 4 == 0 && (uintptr_t)d_out % 4 == 0;
    hipLaunchKernelGGL(remap_kernel, grid_for(out_width, out_height, 1), dim3(kLanesX, kRows), 0, s, d_img, width, height, step, d_mapx, d_mapy,
                       stride, map_vec_ok, out_width, out_height, d_out, out_step, out_vec_ok);
    MLPL_HIP_TRY(hipGetLastError());
    return MLPL_OK;
}

constexpr int kBlockDoubles = 35;   // {K[9], dist[8], Rect[9], Knew[9]}

int launch_fused(mlpl_ctx *ctx, int batch, const uint8_t *d_img1, const uint8_t *d_img2, int width, int height, size_t step, size_t batch_stride,
                 const double *params, int out_width, int out_height, uint8_t *d_out1, uint8_t *d_out2, size_t out_step, size_t out_batch_stride,
                 hipStream_t s) {
    std::vector<MapParams> host((size_t)batch * 2);
    for (size_t i = 0; i < host.size(); ++i) {
        const double *q = params + i * kBlockDoubles;
        if (!make_map_params(q, q + 9, 8, q + 17, q + 26, &host[i])) {
            set_error("rectify_images: parameter block %zu holds a value that is not finite", i);
            return MLPL_E_BAD_INPUT;
        }
    }
    void *dp = nullptr;
    if (int rc = ws_get(ctx, WS_RECTIFY, host.size() * sizeof(MapParams), &dp)) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(dp, host.data(), host.size() * sizeof(MapParams), hipMemcpyHostToDevice, s));
    FusedArgs a{};
    a.img[0] = d_img1, a.img[1] = d_img2, a.out[0] = d_out1, a.out[1] = d_out2;
    a.params = static_cast<const MapParams *>(dp);
    a.step = step, a.batch_stride = batch_stride, a.out_step = out_step, a.out_batch_stride = out_batch_stride;
    a.width = width, a.height = height, a.out_width = out_width, a.out_height = out_height;
    a.out_vec_ok = out_step % 4 == 0 && out_batch_stride % 4 == 0 && (uintptr_t)d_out1 % 4 == 0 && (uintptr_t)d_out2 % 4 == 0;
    hipLaunchKernelGGL(rectify_fused_kernel, grid_for(out_width, out_height, 2 * batch), dim3(kLanesX, kRows), 0, s, a);
    MLPL_HIP_TRY(hipGetLastError());
    return MLPL_OK;
}

bool size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide; }

}  // namespace

}  // namespace mlpl

using namespace mlpl;

extern "C" {

int mlpl_rectify_parameters(const double R[9], const double t_in[3], const double K1[9], const double K2[9], const double *dist1, int n_dist1,
                            const double *dist2, int n_dist2, int width, int height, double alpha, int new_width, int new_height,
                            double Rect1[9], double Rect2[9], double Knew_out[9], int roi[4], double P1[12], double P2[12], double info[8]) try {
    auto n_ok = [](int n) { return n == 0 || n == 4 || n == 5 || n == 8; };
    if (!R || !t_in || !K1 || !K2 || !Rect1 || !Rect2 || !Knew_out || !n_ok(n_dist1) || !n_ok(n_dist2) || (n_dist1 && !dist1) ||
        (n_dist2 && !dist2) || width < 1 || height < 1 || new_width < 0 || new_height < 0 || !finite_all(R, 9) || !finite_all(t_in, 3) ||
        !finite_all(K1, 9) || !finite_all(K2, 9) || (n_dist1 && !finite_all(dist1, n_dist1)) || (n_dist2 && !finite_all(dist2, n_dist2)) ||
        !std::isfinite(alpha) || (t_in[0] == 0.0 && t_in[1] == 0.0 && t_in[2] == 0.0)) {
        set_error("mlpl_rectify_parameters: bad arguments (finite R, t != 0, K1, K2, alpha; 0, 4, 5 or 8 finite coefficients; a positive image "
                  "size; a new size that is not negative)");
        return MLPL_E_BAD_INPUT;
    }
    double k1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, k2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n_dist1; ++i) k1[i] = dist1[i];
    for (int i = 0; i < n_dist2; ++i) k2[i] = dist2[i];
    const int w = width, h = height;
    int nw = new_width, nh = new_height;
    if ((long long)nw * nh == 0) nw = w, nh = h;
    const double nx = (double)w, ny = (double)h;
    // ---- t normalised (:1394-1397)
    double t[3] = {t_in[0], t_in[1], t_in[2]};
    double tn = t[0] * t[0];
    tn = tn + t[1] * t[1];
    tn = tn + t[2] * t[2];
    tn = std::sqrt(tn);
    if (!(tn > 0.0) || !std::isfinite(tn)) {
        set_error("mlpl_rectify_parameters: the norm of t is zero or not finite");
        return MLPL_E_BAD_INPUT;
    }
    if (std::fabs(tn - 1.0) > 1e-4) t[0] = t[0] / tn, t[1] = t[1] / tn, t[2] = t[2] / tn;
    // ---- focal length and first principal point (:1521-1544)
    const int idx = std::fabs(t[0]) > std::fabs(t[1]) ? 0 : 1;
    double fc_new = INFINITY;
    for (int c = 0; c < 2; ++c) {
        const double *A = c == 0 ? K1 : K2;
        const double dk1 = c == 0 ? (n_dist1 ? k1[0] : 0.0) : (n_dist2 ? k2[0] : 0.0);
        double fc = A[4 * (idx ^ 1)];
        if (dk1 < 0) fc = fc * (1.0 + dk1 * (nx * nx + ny * ny) / (4.0 * fc * fc));
        fc_new = fc < fc_new ? fc : fc_new;
    }
    double ccx = (nx - 1.0) / 2.0, ccy = (ny - 1.0) / 2.0;
    ccx = (double)nw * ccx / (double)w;
    ccy = (double)nh * ccy / (double)h;
    double Knew[9] = {fc_new, 0.0, ccx, 0.0, fc_new, ccy, 0.0, 0.0, 1.0};
    // ---- optical centres: c1 = 0, c2 = -(R^T (K2^-1 (K2 t))) (:1549-1550)
    double K2inv[9], a[3], c2[3];
    inv3(K2, K2inv);
    mulv3(K2, t, a);
    mulv3(K2inv, a, a);
    const double Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
    mulv3(Rt, a, c2);
    c2[0] = -c2[0], c2[1] = -c2[1], c2[2] = -c2[2];
    // ---- new axes (:1556-1569)
    const double *v1 = c2;
    const double v2[3] = {-v1[1], v1[0], 0.0};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    double Rv[9];
    for (int r = 0; r < 3; ++r) {
        const double *v = r == 0 ? v1 : (r == 1 ? v2 : v3);
        double n = v[0] * v[0];
        n = n + v[1] * v[1];
        n = n + v[2] * v[2];
        n = std::sqrt(n);
        Rv[3 * r] = v[0] / n, Rv[3 * r + 1] = v[1] / n, Rv[3 * r + 2] = v[2] / n;
    }
    // ---- first pass with K2 (skew 0) as the new matrix: the shift that centres the images (:1572-1610)
    double Kn[9], Po1i[9], Po2i[9], KR[9], Ra[9], Rb[9], tmp[9];
    for (int i = 0; i < 9; ++i) Kn[i] = K2[i];
    Kn[1] = 0.0;
    inv3(K1, Po1i);
    mul3(K2, R, tmp);
    inv3(tmp, Po2i);
    mul3(Kn, Rv, KR);
    mul3(KR, Po1i, Ra);
    mul3(KR, Po2i, Rb);
    const double imc[3] = {(nx - 1.0) / 2.0, (ny - 1.0) / 2.0, 1.0};
    double pa[3], pb[3];
    mulv3(Ra, imc, pa);
    mulv3(Rb, imc, pb);
    const double d1x = imc[0] - pa[0] / pa[2], d1y = imc[1] - pa[1] / pa[2];
    const double d2x = imc[0] - pb[0] / pb[2], d2y = imc[1] - pb[1] / pb[2];
    Knew[2] = Knew[2] + (d1x + d2x) / 2.0;
    Knew[5] = Knew[5] + (d1y + d2y) / 2.0;
    // ---- second pass with Knew, then into 3-D space (:1615-1680)
    double Kni[9], Re1[9], Re2[9];
    mul3(Knew, Rv, KR);
    mul3(KR, Po1i, Ra);
    mul3(KR, Po2i, Rb);
    inv3(Knew, Kni);
    mul3(Ra, K1, tmp);
    mul3(Kni, tmp, Re1);
    mul3(Rb, K2, tmp);
    mul3(Kni, tmp, Re2);
    // ---- principal point from the undistorted corners (:1692-1780)
    int steps[4] = {0, 0, 0, 0};
    double cc[2][2];
    for (int c = 0; c < 2; ++c) {
        const double *A = c == 0 ? K1 : K2, *k = c == 0 ? k1 : k2, *Rk = c == 0 ? Re1 : Re2;
        P2f pts[4];
        steps[c] = corner_points(A, k, nx, ny, pts);
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < 4; ++i) {   // cv::projectPoints, the matrix used directly, t = 0, no distortion
            const double px = (double)pts[i].x, py = (double)pts[i].y;
            const double X = Rk[0] * px + Rk[1] * py + Rk[2];
            const double Y = Rk[3] * px + Rk[4] * py + Rk[5];
            double Z = Rk[6] * px + Rk[7] * py + Rk[8];
            Z = Z != 0 ? 1.0 / Z : 1.0;
            const double u = (X * Z) * fc_new, v = (Y * Z) * fc_new;
            sx = i == 0 ? u : sx + u;
            sy = i == 0 ? v : sy + v;
        }
        cc[c][0] = (nx - 1.0) / 2.0 - sx / 4.0;
        cc[c][1] = (ny - 1.0) / 2.0 - sy / 4.0;
    }
    const double cx0 = (cc[0][0] + cc[1][0]) * 0.5, cy0 = (cc[0][1] + cc[1][1]) * 0.5;
    const double pp[9] = {fc_new, 0.0, cx0, 0.0, fc_new, cy0, 0.0, 0.0, 1.0};
    alpha = std::min(alpha, 1.0);
    Rectf inner1, outer1, inner2, outer2;
    steps[2] = rectangles(K1, k1, Re1, pp, w, h, &inner1, &outer1);
    steps[3] = rectangles(K2, k2, Re2, pp, w, h, &inner2, &outer2);
    const double cx1 = (double)nw * cx0 / (double)w, cy1 = (double)nh * cy0 / (double)h;
    double s = 1.0, s0 = 0.0, s1 = 0.0;
    if (alpha >= 0) {
        s0 = std::max(std::max(std::max(cx1 / (cx0 - inner1.x), cy1 / (cy0 - inner1.y)), ((double)nw - cx1) / ((double)(inner1.x + inner1.width) - cx0)),
                      ((double)nh - cy1) / ((double)(inner1.y + inner1.height) - cy0));
        s1 = std::min(std::min(std::min(cx1 / (cx0 - outer1.x), cy1 / (cy0 - outer1.y)), ((double)nw - cx1) / ((double)(outer1.x + outer1.width) - cx0)),
                      ((double)nh - cy1) / ((double)(outer1.y + outer1.height) - cy0));
        s = s0 * (1.0 - alpha) + s1 * alpha;
        if (s > 2.0 || s < 0.5) s = 1.0;
    }
    if (info) {
        info[0] = fc_new, info[1] = s0, info[2] = s1, info[3] = s;
        for (int i = 0; i < 4; ++i) info[4 + i] = (double)steps[i];
    }
    const double fc_s = fc_new * s;
    const double Kout[9] = {fc_s, 0.0, cx1, 0.0, fc_s, cy1, 0.0, 0.0, 1.0};
    if (roi) {   // (:1819-1823) and cv::Rect & cv::Rect(0, 0, nw, nh), the sums in 64 bits
        const long long rx = sat_int(std::ceil(((double)inner1.x - cx0) * s + cx1)), ry = sat_int(std::ceil(((double)inner1.y - cy0) * s + cy1));
        const long long rw = sat_int(std::floor((double)inner1.width * s)), rh = sat_int(std::floor((double)inner1.height * s));
        const long long x1 = std::max(rx, 0LL), y1 = std::max(ry, 0LL);
        const long long ww = std::min(rx + rw, (long long)nw) - x1, hh = std::min(ry + rh, (long long)nh) - y1;
        if (ww > 0 && hh > 0) roi[0] = (int)x1, roi[1] = (int)y1, roi[2] = (int)ww, roi[3] = (int)hh;
        else roi[0] = roi[1] = roi[2] = roi[3] = 0;
    }
    for (int i = 0; i < 9; ++i) Rect1[i] = Re1[i], Rect2[i] = Re2[i], Knew_out[i] = Kout[i];
    for (int c = 0; c < 2; ++c) {
        double *P = c == 0 ? P1 : P2;
        if (!P) continue;
        const double zero[3] = {0.0, 0.0, 0.0};
        double tc[3];
        mulv3(Rv, c == 0 ? zero : c2, tc);
        const double Pt[12] = {Rv[0], Rv[1], Rv[2], -tc[0], Rv[3], Rv[4], Rv[5], -tc[1], Rv[6], Rv[7], Rv[8], -tc[2]};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                double q = Kout[3 * i] * Pt[j];
                q = q + Kout[3 * i + 1] * Pt[4 + j];
                q = q + Kout[3 * i + 2] * Pt[8 + j];
                P[4 * i + j] = q;
            }
    }
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_rectify_parameters")

int mlpl_rectify_maps_dev(mlpl_ctx *ctx, const double K[9], const double *dist, int n_dist, const double Rect[9], const double Knew[9],
                          int width, int height, float *d_mapx, float *d_mapy, size_t map_stride, void *stream) try {
    MapParams p;
    if (!ctx || !K || !Rect || !Knew || !(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8) || (n_dist && !dist) || !size_ok(width, height) ||
        !d_mapx || !d_mapy || map_stride < (size_t)width || !make_map_params(K, dist, n_dist, Rect, Knew, &p)) {
        set_error("mlpl_rectify_maps: bad arguments (finite K, Rect, Knew; 0, 4, 5 or 8 finite coefficients; sides in [1, 16384]; row stride >= width)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_maps(p, width, height, d_mapx, d_mapy, map_stride, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_rectify_maps_dev")

int mlpl_rectify_maps(mlpl_ctx *ctx, const double K[9], const double *dist, int n_dist, const double Rect[9], const double Knew[9], int width,
                      int height, float *mapx, float *mapy) try {
    if (!ctx || !mapx || !mapy || !size_ok(width, height)) {
        set_error("mlpl_rectify_maps: bad arguments (sides in [1, 16384], two output maps)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const size_t stride = ((size_t)width + 3) & ~size_t(3), bytes = stride * (size_t)height * sizeof(float);
    void *dx, *dy;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX4, bytes, &dx))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, bytes, &dy))) return rc;
    if ((rc = mlpl_rectify_maps_dev(ctx, K, dist, n_dist, Rect, Knew, width, height, (float *)dx, (float *)dy, stride, ctx->stream))) return rc;
    MLPL_HIP_TRY(hipMemcpy2DAsync(mapx, (size_t)width * 4, dx, stride * 4, (size_t)width * 4, (size_t)height, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipMemcpy2DAsync(mapy, (size_t)width * 4, dy, stride * 4, (size_t)width * 4, (size_t)height, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_rectify_maps")

int mlpl_remap_bilinear_dev(mlpl_ctx *ctx, const uint8_t *d_img, int width, int height, size_t step, const float *d_mapx, const float *d_mapy,
                            size_t map_stride, int out_width, int out_height, uint8_t *d_out, size_t out_step, void *stream) try {
    if (!ctx || !d_img || !size_ok(width, height) || step < (size_t)width || !d_mapx || !d_mapy || !size_ok(out_width, out_height) ||
        map_stride < (size_t)out_width || !d_out || out_step < (size_t)out_width) {
        set_error("mlpl_remap_bilinear: bad arguments (8-bit image and output with sides in [1, 16384], row step >= width, map stride >= output width)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_remap(d_img, width, height, step, d_mapx, d_mapy, map_stride, out_width, out_height, d_out, out_step, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_remap_bilinear_dev")

int mlpl_remap_bilinear(mlpl_ctx *ctx, const uint8_t *img, int width, int height, size_t step, const float *mapx, const float *mapy, int out_width,
                        int out_height, uint8_t *out, size_t out_step) try {
    if (!ctx || !img || !size_ok(width, height) || step < (size_t)width || !mapx || !mapy || !size_ok(out_width, out_height) || !out ||
        out_step < (size_t)out_width) {
        set_error("mlpl_remap_bilinear: bad arguments (8-bit image and output with sides in [1, 16384], row step >= width)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t mstride = ((size_t)out_width + 3) & ~size_t(3), ostep = mstride;
    void *di, *dx, *dy, *dout;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, (size_t)width * height, &di))) return rc;
    if ((rc = ws_get(ctx, WS_AUX2, ostep * (size_t)out_height, &dout))) return rc;
    if ((rc = ws_get(ctx, WS_AUX4, mstride * (size_t)out_height * 4, &dx))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, mstride * (size_t)out_height * 4, &dy))) return rc;
    MLPL_HIP_TRY(hipMemcpy2DAsync(di, (size_t)width, img, step, (size_t)width, (size_t)height, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpy2DAsync(dx, mstride * 4, mapx, (size_t)out_width * 4, (size_t)out_width * 4, (size_t)out_height, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpy2DAsync(dy, mstride * 4, mapy, (size_t)out_width * 4, (size_t)out_width * 4, (size_t)out_height, hipMemcpyHostToDevice, s));
    if ((rc = launch_remap((const uint8_t *)di, width, height, (size_t)width, (const float *)dx, (const float *)dy, mstride, out_width, out_height,
                           (uint8_t *)dout, ostep, s)))
        return rc;
    MLPL_HIP_TRY(hipMemcpy2DAsync(out, out_step, dout, ostep, (size_t)out_width, (size_t)out_height, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_remap_bilinear")

int mlpl_rectify_images_dev(mlpl_ctx *ctx, int batch, const uint8_t *d_img1, const uint8_t *d_img2, int width, int height, size_t step,
                            size_t batch_stride, const double *params, int out_width, int out_height, uint8_t *d_out1, uint8_t *d_out2,
                            size_t out_step, size_t out_batch_stride, void *stream) try {
    if (!ctx || batch < 1 || batch > 32767 || !d_img1 || !d_img2 || !size_ok(width, height) || step < (size_t)width ||
        (batch > 1 && batch_stride < step * (size_t)height) || !params || !size_ok(out_width, out_height) || !d_out1 || !d_out2 ||
        out_step < (size_t)out_width || (batch > 1 && out_batch_stride < out_step * (size_t)out_height)) {
        set_error("mlpl_rectify_images_dev: bad arguments (batch in [1, 32767]; 8-bit images and outputs with sides in [1, 16384], row step >= "
                  "width, batch stride >= step * height)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_fused(ctx, batch, d_img1, d_img2, width, height, step, batch_stride, params, out_width, out_height, d_out1, d_out2, out_step,
                        out_batch_stride, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_rectify_images_dev")

int mlpl_rectify_images(mlpl_ctx *ctx, const uint8_t *img1, const uint8_t *img2, int width, int height, size_t step, const double *params,
                        int out_width, int out_height, uint8_t *out1, uint8_t *out2, size_t out_step) try {
    if (!ctx || !img1 || !img2 || !size_ok(width, height) || step < (size_t)width || !params || !size_ok(out_width, out_height) || !out1 || !out2 ||
        out_step < (size_t)out_width) {
        set_error("mlpl_rectify_images: bad arguments (8-bit images and outputs with sides in [1, 16384], row step >= width)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t ostep = ((size_t)out_width + 3) & ~size_t(3);
    void *d1, *d2, *o1, *o2;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, (size_t)width * height, &d1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, (size_t)width * height, &d2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX2, ostep * (size_t)out_height, &o1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX3, ostep * (size_t)out_height, &o2))) return rc;
    MLPL_HIP_TRY(hipMemcpy2DAsync(d1, (size_t)width, img1, step, (size_t)width, (size_t)height, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpy2DAsync(d2, (size_t)width, img2, step, (size_t)width, (size_t)height, hipMemcpyHostToDevice, s));
    if ((rc = launch_fused(ctx, 1, (const uint8_t *)d1, (const uint8_t *)d2, width, height, (size_t)width, 0, params, out_width, out_height,
                           (uint8_t *)o1, (uint8_t *)o2, ostep, 0, s)))
        return rc;
    MLPL_HIP_TRY(hipMemcpy2DAsync(out1, out_step, o1, ostep, (size_t)out_width, (size_t)out_height, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpy2DAsync(out2, out_step, o2, ostep, (size_t)out_width, (size_t)out_height, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_rectify_images")

}  // extern "C"

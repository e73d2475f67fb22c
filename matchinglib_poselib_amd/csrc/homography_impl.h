// homography_impl.h -- poselib::computeHomographyArrsac / estimateMultHomographys (poselib/source/pose_homography.cpp:291-885) on the MI355X.
// Included by ransac_5pt.hip inside namespace mlpl after batch_hub.h and arrsac_impl.h: HomogRun is the homography side of that file's
// ArrsacTemplate (the sequential ARRSAC program, written once for both estimators), the batch entries are callers of the hub's cohort / lane
// driver (hub_batch_drive), and the sample kernel uses ransac_5pt.hip's jacobi9_wave.
//
// The estimator is the same theia::Arrsac template the essential-matrix path runs, constructed as Arrsac(4, th^2, 500, 100, 12)
// (pose_homography.cpp:505): minimal sample 4, at most 500 hypotheses, blocks of 100, inner RANSAC on min(12, max_inl / 2) points with the
// non-minimal estimator unless that size is 4.  ONE model per sample.  As for E, the host runs the reference's control flow literally on
// inlier bit rows and sends the samples it will need to the device in speculative batches (arrsac_impl.h explains why a wrong guess costs a
// batch and never a result).  All arithmetic is fp64; no matrix cores.  Every kernel is a body(const Args &, block x, block y) registered with
// MLPL_HUB_KERNEL (batch_hub.h): a run issues its launches through a Launcher, which launches on the caller's stream (a call alone) or records
// them for the hub (mlpl_homography_arrsac_batch_dev / mlpl_mult_homographies_batch_dev: every problem a fiber, the launches of the runs at
// the same point of their control flow merged, blockIdx.z = the run).  Both instantiations come from the one body, so a problem's results
// do not depend on how it was launched.  The kernels (homog_<name>_body in the code, HK_HOM_* in hub_kernels.h):
//   homog_sample_kernel   one wave per sample: runHomogrophyKernel (:674-744) -- centroid / mean absolute deviation, LtL summed in the
//                         reference's point order, eigenvector of the smallest eigenvalue (jacobi9_wave), denormalise, scale by 1 / H(2,2);
//                         samples of more than 4 points are cv::findHomography(m1, m2, 0): float32 points, the same DLT, LMSolver's 10
//                         turns on the 8 free parameters, then the reference's H(0,0) == 0 || H(2,2) == 0 rejection (:627)
//   homog_check_kernel    one wave per model: inlier bits (transfer error < th^2, strict) of the first min(n, 1024) correspondences
//   homog_extend_kernel   the same bits over all n for the few models that survive past correspondence 1024 (on demand)
//   homog_inliers_kernel  findHomographyInliers (:785-813): mask (err <= th^2) over all n, counts, order-preserving compaction of the
//                         inliers (for the refinement) and of the outliers (the next plane's input) -- one workgroup, a fixed-order scan
//   homog_refine_kernel   refineHomography (:825-885): the CvLevMarq state machine in one launch, one workgroup, fixed-order sums
// cv::eigen, LMSolver::run and CvLevMarq::updateAlt / step are restated from OpenCV 4.x; the damped 8 x 8 systems are solved by Gaussian
// elimination with partial pivoting (nothing pins OpenCV's DECOMP_EIG / DECOMP_SVD).  Pinned by tests: this code against the sequential
// restatement tests/cpp/homography_oracle.cpp; not pinned: that restatement against a build of the reference or of OpenCV.

namespace {

constexpr int kHomMinSample = 4;
constexpr int kHomMaxSample = 12;
constexpr int kHomBatchCap = 512;
constexpr int kHomPoolSamples = 8192;
constexpr int kHomInlThreads = 1024;
constexpr int kHomRefineThreads = 256;

// element j of the two DLT rows of a normalised correspondence: Lx = {X, Y, 1, 0, 0, 0, -x X, -x Y, -x}, Ly = {0, 0, 0, X, Y, 1, -y X, -y Y, -y}
__device__ __forceinline__ double hom_row_elem(int which, int j, double X, double Y, double x, double y) {
    const int g = j / 3, r = j - g * 3;
    const double base = r == 0 ? X : (r == 1 ? Y : 1.0);
    if (g == 2) return r == 2 ? -(which ? y : x) : -(which ? y : x) * base;
    return g == which ? base : 0.0;
}

__device__ __forceinline__ void hom_mat3_mul(const double *a, const double *b, double *c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
            c[i * 3 + j] = s;
        }
}

// residual and Jacobian rows of the transfer error of one correspondence under the 8 parameters h (refineHomography / HomographyRefineCallback)
__device__ __forceinline__ void hom_point_jac(const double *h, double Mx, double My, double mx, double my, double *J0, double *J1, double *err) {
    double ww = h[6] * Mx + h[7] * My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
    const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
    const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    err[0] = xi - mx, err[1] = yi - my;
    J0[0] = Mx * ww, J0[1] = My * ww, J0[2] = ww, J0[3] = 0, J0[4] = 0, J0[5] = 0, J0[6] = -Mx * ww * xi, J0[7] = -My * ww * xi;
    J1[0] = 0, J1[1] = 0, J1[2] = 0, J1[3] = Mx * ww, J1[4] = My * ww, J1[5] = ww, J1[6] = -Mx * ww * yi, J1[7] = -My * ww * yi;
}

// The same residual with the products and sums of the two projective rows carried as unevaluated pairs (error-free product and sum), for
// refineHomography's cost.  At pixel coordinates x_i = (h0 Mx + h1 My + h2) ww carries ~1e-13 of rounding, the residual x_i - m.x cancels
// three digits, and |err|^2 summed over a few thousand inliers is then noisy at ~3e-12 -- the size of the cost decrease of the LAST
// Gauss-Newton step that still matters (~1e-10 of H away from the fixed point).  CvLevMarq accepts a step iff the cost did not rise, so with
// plain doubles that step is a coin flip: a run of rejections raises lambda until the step vanishes, the relative-change test fires and H
// stays ~1e-9 short (the reference itself does this on about one pixel-unit scene in twenty, as does the sequential restatement: DESIGN 8).
// With these residuals the cost is exact to the rounding of its sum (~1e-13) and the decision is taken by the cost.
__device__ __forceinline__ void hom_two_prod(double a, double b, double &hi, double &lo) {
    hi = a * b;
    lo = fma(a, b, -hi);
}
__device__ __forceinline__ void hom_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void hom_affine_dd(double a, double x, double b, double y, double c, double &hi, double &lo) {  // a x + b y + c
    double p1, e1, p2, e2, s1, f1, s2, f2;
    hom_two_prod(a, x, p1, e1);
    hom_two_prod(b, y, p2, e2);
    hom_two_sum(p1, p2, s1, f1);
    hom_two_sum(s1, c, s2, f2);
    hi = s2, lo = (f1 + f2) + (e1 + e2);
}
__device__ __forceinline__ double hom_residual_dd(double nh, double nl, double dh, double dl, double target) {  // (nh + nl) / (dh + dl) - target
    const double q = nh / dh;
    const double r = (fma(-q, dh, nh) + nl) - q * dl;
    return (q - target) + r / dh;
}
__device__ __forceinline__ void hom_point_err_exact(const double *h, double Mx, double My, double mx, double my, double *err) {
    double dh, dl, nh, nl;
    hom_affine_dd(h[6], Mx, h[7], My, 1., dh, dl);
    if (!(fabs(dh) > DBL_EPSILON)) {  // the reference's guard: ww = 0
        err[0] = 0 - mx, err[1] = 0 - my;
        return;
    }
    hom_affine_dd(h[0], Mx, h[1], My, h[2], nh, nl);
    err[0] = hom_residual_dd(nh, nl, dh, dl, mx);
    hom_affine_dd(h[3], Mx, h[4], My, h[5], nh, nl);
    err[1] = hom_residual_dd(nh, nl, dh, dl, my);
}

// 8 x 8 system by Gaussian elimination with partial pivoting, one lane; A (row-major) and b are destroyed.  All three live in LDS.
__device__ __noinline__ void hom_solve8(double *A, double *b, double *x) {
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        for (int r = c + 1; r < 8; ++r)
            if (fabs(A[r * 8 + c]) > fabs(A[piv * 8 + c])) piv = r;
        if (piv != c) {
            for (int k = 0; k < 8; ++k) {
                const double t = A[c * 8 + k];
                A[c * 8 + k] = A[piv * 8 + k], A[piv * 8 + k] = t;
            }
            const double t = b[c];
            b[c] = b[piv], b[piv] = t;
        }
        const double inv = 1.0 / A[c * 8 + c];
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r * 8 + c] * inv;
            for (int k = c; k < 8; ++k) A[r * 8 + k] -= f * A[c * 8 + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = 7; r >= 0; --r) {
        double s = b[r];
        for (int k = r + 1; k < 8; ++k) s -= A[r * 8 + k] * x[k];
        x[r] = s / A[r * 8 + r];
    }
}

struct HomLmLds {  // LMSolver's state of one sample (lane 0 works on it)
    double x[8], xd[8], A[64], v[8], D[8], Ap[64], rhs[8], d[8], col[8];
};

// J^T J (full), J^T r, |r|^2 and |r|_inf over the m points of a sample (pts[i] = {Mx, My, mx, my}), in point order; A == nullptr: residuals only
__device__ __noinline__ void hom_sample_sums(const double (*pts)[4], int m, const double *h, double *A, double *v, double *S, double *rinf) {
    if (A) {
        for (int k = 0; k < 64; ++k) A[k] = 0;
        for (int k = 0; k < 8; ++k) v[k] = 0;
    }
    double en = 0, ri = 0;
    for (int i = 0; i < m; ++i) {
        double J0[8], J1[8], err[2];
        hom_point_jac(h, pts[i][0], pts[i][1], pts[i][2], pts[i][3], J0, J1, err);
        if (A) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
#pragma unroll
                for (int k = j; k < 8; ++k) A[j * 8 + k] += J0[j] * J0[k] + J1[j] * J1[k];
                v[j] += J0[j] * err[0] + J1[j] * err[1];
            }
        }
        en += err[0] * err[0] + err[1] * err[1];
        if (fabs(err[0]) > ri) ri = fabs(err[0]);
        if (fabs(err[1]) > ri) ri = fabs(err[1]);
    }
    if (A)
        for (int j = 0; j < 8; ++j)
            for (int k = 0; k < j; ++k) A[j * 8 + k] = A[k * 8 + j];
    *S = en;
    if (rinf) *rinf = ri;
}

// LMSolver::run (OpenCV 4.x levmarq.cpp) as cv::findHomography drives it: 10 turns at most, epsx = epsf = FLT_EPSILON; h: 8 parameters
__device__ __noinline__ void hom_lm_polish(const double (*pts)[4], int m, double *h, HomLmLds &W) {
    double S, rinf;
    for (int i = 0; i < 8; ++i) W.x[i] = h[i];
    hom_sample_sums(pts, m, W.x, W.A, W.v, &S, &rinf);
    for (int i = 0; i < 8; ++i) W.D[i] = W.A[i * 8 + i];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        for (int k = 0; k < 64; ++k) W.Ap[k] = W.A[k];
        for (int i = 0; i < 8; ++i) W.Ap[i * 8 + i] += lambda * W.D[i], W.rhs[i] = W.v[i];
        hom_solve8(W.Ap, W.rhs, W.d);
        for (int i = 0; i < 8; ++i) W.xd[i] = W.x[i] - W.d[i];
        double Sd;
        hom_sample_sums(pts, m, W.xd, nullptr, nullptr, &Sd, nullptr);
        double dS = 0, t = 0;
        for (int i = 0; i < 8; ++i) {
            double td = 2 * W.v[i];
            for (int k = 0; k < 8; ++k) td -= W.A[i * 8 + k] * W.d[k];
            dS += W.d[i] * td;
            t += W.d[i] * W.v[i];
        }
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = fmin(fmax(nu, 2.), 10.);
            if (lambda == 0) {
                double maxval = DBL_EPSILON;
                for (int c = 0; c < 8; ++c) {  // the diagonal of A^-1
                    for (int k = 0; k < 64; ++k) W.Ap[k] = W.A[k];
                    for (int k = 0; k < 8; ++k) W.rhs[k] = k == c ? 1.0 : 0.0;
                    hom_solve8(W.Ap, W.rhs, W.col);
                    maxval = fmax(maxval, fabs(W.col[c]));
                }
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
            for (int i = 0; i < 8; ++i) W.x[i] = W.xd[i];
            hom_sample_sums(pts, m, W.x, W.A, W.v, &S, &rinf);
        }
        iter++;
        double dinf = 0;
        for (int i = 0; i < 8; ++i)
            if (fabs(W.d[i]) > dinf) dinf = fabs(W.d[i]);
        const bool proceed = iter < 10 && dinf >= (double)FLT_EPSILON && rinf >= (double)FLT_EPSILON;
        if (!proceed) break;
    }
    for (int i = 0; i < 8; ++i) h[i] = W.x[i];
}

// One wave per sample: smp[b] = {m, idx[1..14], kind} (ArrKey's layout); H_out[b][9], ok_out[b].  The host has checked 4 <= m <= 12 and
// every index against n.
struct HomSampleArgs {
    KHdr hdr;
    const double *p1, *p2;
    const int32_t *smp;
    int n_samples;
    double *H_out;
    int32_t *ok_out;
};
__device__ __forceinline__ void homog_sample_body(const HomSampleArgs &a, int bx, int) {
    const double *__restrict__ p1 = a.p1, *__restrict__ p2 = a.p2;
    const int32_t *__restrict__ smp = a.smp;
    double *__restrict__ H_out = a.H_out;
    int32_t *__restrict__ ok_out = a.ok_out;
    const int n_samples = a.n_samples;
    __shared__ Jacobi9Lds J;
    __shared__ HomLmLds W;
    __shared__ double xs[kHomMaxSample][4];  // {Mx, My, mx, my}
    __shared__ double nrm[8];                // cM, sM, cm, sm (x, y each)
    __shared__ int s_ok;
    const int lane = threadIdx.x, b = bx;
    if (b >= n_samples) return;
    const int32_t *sm = smp + (size_t)b * kArrSmpStride;
    const int m = sm[0];
    const bool nonmin = m > kHomMinSample;
    if (lane < m) {
        const int idx = sm[1 + lane];
        double Mx = p1[2 * idx], My = p1[2 * idx + 1], mx = p2[2 * idx], my = p2[2 * idx + 1];
        if (nonmin) Mx = (double)(float)Mx, My = (double)(float)My, mx = (double)(float)mx, my = (double)(float)my;  // findHomography works on Point2f
        xs[lane][0] = Mx, xs[lane][1] = My, xs[lane][2] = mx, xs[lane][3] = my;
    }
    wave_sync();
    if (lane == 0) {
        double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
        for (int i = 0; i < m; ++i) {
            cmx += xs[i][2], cmy += xs[i][3];
            cMx += xs[i][0], cMy += xs[i][1];
        }
        cmx /= m, cmy /= m, cMx /= m, cMy /= m;
        for (int i = 0; i < m; ++i) {
            smx += fabs(xs[i][2] - cmx), smy += fabs(xs[i][3] - cmy);
            sMx += fabs(xs[i][0] - cMx), sMy += fabs(xs[i][1] - cMy);
        }
        s_ok = !(fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON);
        nrm[0] = cMx, nrm[1] = cMy, nrm[2] = m / sMx, nrm[3] = m / sMy;
        nrm[4] = cmx, nrm[5] = cmy, nrm[6] = m / smx, nrm[7] = m / smy;
    }
    wave_sync();
    if (!s_ok) {
        if (lane < 9) H_out[(size_t)b * 9 + lane] = 0.0;
        if (lane == 0) ok_out[b] = 0;
        return;
    }
    for (int e = lane; e < 81; e += 64) {
        const int a = e / 9, c = e - a * 9;
        const int j = a < c ? a : c, k = a < c ? c : a;
        double acc = 0;
        for (int i = 0; i < m; ++i) {
            const double X = (xs[i][0] - nrm[0]) * nrm[2], Y = (xs[i][1] - nrm[1]) * nrm[3];
            const double x = (xs[i][2] - nrm[4]) * nrm[6], y = (xs[i][3] - nrm[5]) * nrm[7];
            acc += hom_row_elem(0, j, X, Y, x, y) * hom_row_elem(0, k, X, Y, x, y) + hom_row_elem(1, j, X, Y, x, y) * hom_row_elem(1, k, X, Y, x, y);
        }
        J.G[a][c] = acc;
        J.Vv[a][c] = (a == c) ? 1.0 : 0.0;
    }
    wave_sync();
    jacobi9_wave(J, lane);
    wave_sync();
    if (lane == 0) {
        int order[9];
        order_desc9(J, order);
        double H0[9], Ht[9], Hd[9], H[9];
        for (int k = 0; k < 9; ++k) H0[k] = J.Vv[k][order[8]];
        const double invHnorm[9] = {1. / nrm[6], 0, nrm[4], 0, 1. / nrm[7], nrm[5], 0, 0, 1};
        const double Hnorm2[9] = {nrm[2], 0, -nrm[0] * nrm[2], 0, nrm[3], -nrm[1] * nrm[3], 0, 0, 1};
        hom_mat3_mul(invHnorm, H0, Ht);
        hom_mat3_mul(Ht, Hnorm2, Hd);
        const double inv = 1. / Hd[8];  // no guard, as the reference: a degenerate sample yields a non-finite model
        for (int k = 0; k < 9; ++k) H[k] = Hd[k] * inv;
        int ok = 1;
        if (nonmin) {
            hom_lm_polish(xs, m, H, W);
            if (H[0] == 0.0 || H[8] == 0.0) ok = 0;
        }
        for (int k = 0; k < 9; ++k) H_out[(size_t)b * 9 + k] = H[k];
        ok_out[b] = ok;
    }
}
MLPL_HUB_KERNEL(HK_HOM_SAMPLE, HomSampleArgs, homog_sample_body, 64);

struct HomPackArgs {  // 256 threads per block
    KHdr hdr;
    const double *p1, *p2;
    int n;
    double4 *pts;
};
__device__ __forceinline__ void homog_pack_body(const HomPackArgs &a, int bx, int) {
    const int i = bx * 256 + threadIdx.x;
    if (i < a.n) a.pts[i] = make_double4(a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1]);
}
MLPL_HUB_KERNEL(HK_HOM_PACK, HomPackArgs, homog_pack_body, 256);
// the winner's matrix and the counts of the inlier pass, for the host (mapped block)
struct HomFinalArgs {
    KHdr hdr;
    const double *H;
    const int32_t *counts;
    double *H_out;
    int32_t *counts_out;
};
__device__ __forceinline__ void homog_final_body(const HomFinalArgs &a, int, int) {
    const int t = threadIdx.x;
    if (t < 9) a.H_out[t] = a.H[t];
    if (t < 2) a.counts_out[t] = a.counts[t];
}
MLPL_HUB_KERNEL(HK_HOM_FINAL, HomFinalArgs, homog_final_body, 64);

// ArrHomogrophyEstimator::Error (pose_homography.cpp:642-663)
__device__ __forceinline__ double hom_transfer_err(const double *H, double Mx, double My, double mx, double my) {
    const double ww = 1. / (H[6] * Mx + H[7] * My + 1.);
    const double dx = (H[0] * Mx + H[1] * My + H[2]) * ww - mx;
    const double dy = (H[3] * Mx + H[4] * My + H[5]) * ww - my;
    return dx * dx + dy * dy;
}

// One wave per model: bit i of its row = Error(i) < thresh2 for i < flag_points <= 1024 (16 ballot words, the layout of arrsac_check_kernel);
// the rows and the validity words go straight to the mapped host block.
struct HomCheckArgs {
    KHdr hdr;
    const double4 *pts;
    int flag_points;
    const double *H_tab;
    const int32_t *ok_tab;
    int n_models;
    double thresh2;
    unsigned long long *out_rows;
    int32_t *out_ok;
};
__device__ __forceinline__ void homog_check_body(const HomCheckArgs &a, int bx, int) {
    const double4 *__restrict__ pts = a.pts;
    const double *__restrict__ H_tab = a.H_tab;
    const int32_t *__restrict__ ok_tab = a.ok_tab;
    unsigned long long *__restrict__ out_rows = a.out_rows;
    int32_t *__restrict__ out_ok = a.out_ok;
    const int flag_points = a.flag_points, n_models = a.n_models;
    const double thresh2 = a.thresh2;
    const int lane = threadIdx.x, b = bx;
    if (b >= n_models) return;
    const int ok = ok_tab[b];
    if (lane == 0) out_ok[b] = ok;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = H_tab[(size_t)b * 9 + k];
#pragma unroll
    for (int w = 0; w < kArrFlagWords; ++w) {
        const int i = w * 64 + lane;
        bool in = false;
        if (ok && i < flag_points) {
            const double4 p = pts[i];
            in = hom_transfer_err(h, p.x, p.y, p.z, p.w) < thresh2;
        }
        const unsigned long long bal = __ballot(in);
        if (lane == 0) out_rows[(size_t)b * kArrFlagWords + w] = bal;
    }
}
MLPL_HUB_KERNEL(HK_HOM_CHECK, HomCheckArgs, homog_check_body, 64);

// Inlier bits of table models over ALL n correspondences (the preemptive stage past the first 1024: reached when the hypothesis set keeps
// growing instead of halving -- inlier ratios above ~0.9, where the initial set is tiny and every block of 100 generates half of what is
// missing to 500, so the first halving comes at correspondence 1100): out[i] = words_full ballot words for table row rows[i].
struct HomExtendArgs {
    KHdr hdr;
    const int32_t *rows;
    int n_rows;
    const double4 *pts;
    int n, words_full;
    const double *H_tab;
    double thresh2;
    unsigned long long *out;
};
__device__ __forceinline__ void homog_extend_body(const HomExtendArgs &a, int bx, int) {
    const int32_t *__restrict__ rows = a.rows;
    const double4 *__restrict__ pts = a.pts;
    const double *__restrict__ H_tab = a.H_tab;
    unsigned long long *__restrict__ out = a.out;
    const int n_rows = a.n_rows, n = a.n, words_full = a.words_full;
    const double thresh2 = a.thresh2;
    const int i = bx, lane = threadIdx.x;
    if (i >= n_rows) return;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = H_tab[(size_t)rows[i] * 9 + k];
    for (int w = 0; w < words_full; ++w) {
        const int j = w * 64 + lane;
        bool in = false;
        if (j < n) {
            const double4 p = pts[j];
            in = hom_transfer_err(h, p.x, p.y, p.z, p.w) < thresh2;
        }
        const unsigned long long bal = __ballot(in);
        if (lane == 0) out[(size_t)i * words_full + w] = bal;
    }
}
MLPL_HUB_KERNEL(HK_HOM_EXTEND, HomExtendArgs, homog_extend_body, 64);

// findHomographyInliers with one model over all n correspondences, one workgroup: mask[i] = !(err > th2) (the reference clears a point when
// err > th2), the round's label for its inliers in the caller's original indexing (label_orig[orig_in[i]] = label, optional), the inliers compacted in order as
// {Mx, My, mx, my} rows (in_pts), the outliers compacted in order with their original indices (out_p1 / out_p2 / out_orig, optional), and
// counts = {inliers, outliers}.  Chunks of 1024 points; positions from ballots and a fixed-order scan over the waves' counts.
struct HomInliersArgs {  // one workgroup of kHomInlThreads
    KHdr hdr;
    const double *p1, *p2;
    int n;
    const double *H;
    double th2;
    int force_all;
    uint8_t *mask;
    const int32_t *orig_in;
    int32_t *label_orig;
    int label;
    double4 *in_pts;
    double *out_p1, *out_p2;
    int32_t *out_orig, *counts;
};
__device__ __forceinline__ void homog_inliers_body(const HomInliersArgs &a, int, int) {
    const double *__restrict__ p1 = a.p1, *__restrict__ p2 = a.p2, *__restrict__ H = a.H;
    uint8_t *__restrict__ mask = a.mask;
    const int32_t *__restrict__ orig_in = a.orig_in;
    int32_t *__restrict__ label_orig = a.label_orig, *__restrict__ out_orig = a.out_orig, *__restrict__ counts = a.counts;
    double4 *__restrict__ in_pts = a.in_pts;
    double *__restrict__ out_p1 = a.out_p1, *__restrict__ out_p2 = a.out_p2;
    const int n = a.n, force_all = a.force_all, label = a.label;
    const double th2 = a.th2;
    __shared__ int wcount[kHomInlThreads / 64];
    __shared__ int s_base_in, s_base_out;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = H[k];
    if (tid == 0) s_base_in = 0, s_base_out = 0;
    __syncthreads();
    for (int start = 0; start < n; start += kHomInlThreads) {
        const int i = start + tid;
        const bool valid = i < n;
        double Mx = 0, My = 0, mx = 0, my = 0;
        bool in = false;
        if (valid) {
            Mx = p1[2 * i], My = p1[2 * i + 1], mx = p2[2 * i], my = p2[2 * i + 1];
            in = force_all || !(hom_transfer_err(h, Mx, My, mx, my) > th2);
        }
        const unsigned long long bal = __ballot(in);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int wbase = 0, total = 0;
        for (int w = 0; w < kHomInlThreads / 64; ++w) {
            const int c = wcount[w];
            if (w < wave) wbase += c;
            total += c;
        }
        const int in_before = wbase + before;  // inliers of this chunk in front of point i
        const int base_in = s_base_in, base_out = s_base_out;
        if (valid) {
            if (mask) mask[i] = in ? 1 : 0;
            const int oi = orig_in ? orig_in[i] : i;
            if (label_orig && in) label_orig[oi] = label;
            if (in) {
                if (in_pts) in_pts[base_in + in_before] = make_double4(Mx, My, mx, my);
            } else if (out_p1) {
                const int pos = base_out + (tid - in_before);
                out_p1[2 * pos] = Mx, out_p1[2 * pos + 1] = My;
                out_p2[2 * pos] = mx, out_p2[2 * pos + 1] = my;
                out_orig[pos] = oi;
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int nv = min(kHomInlThreads, n - start);
            s_base_in = base_in + total, s_base_out = base_out + (nv - total);
        }
        __syncthreads();
    }
    if (tid == 0) counts[0] = s_base_in, counts[1] = s_base_out;
}
MLPL_HUB_KERNEL(HK_HOM_INLIERS, HomInliersArgs, homog_inliers_body, kHomInlThreads);

// refineHomography (pose_homography.cpp:825-885): CvLevMarq(8, 0, {max_iters, DBL_EPSILON}) driven through updateAlt, all of it in one
// launch of one workgroup.  Every evaluation adds the 36 + 8 + 1 sums (upper triangle of J^T J, J^T err, |err|^2) over the inliers in a
// fixed order: a thread walks its points in index order, the wave folds by butterfly, thread k adds the waves' partial sums in wave order.
// Thread 0 runs the state machine and solves the damped 8 x 8 system.  out[0..8] = the refined matrix (H(2,2) copied from H_in).
struct HomRefineArgs {  // one workgroup of kHomRefineThreads
    KHdr hdr;
    const double4 *in_pts;
    const int32_t *count_ptr;
    const double *H_in;
    int max_iters;
    double *out;
};
__device__ __forceinline__ void homog_refine_body(const HomRefineArgs &a, int, int) {
    const double4 *__restrict__ in_pts = a.in_pts;
    const int32_t *__restrict__ count_ptr = a.count_ptr;
    const double *__restrict__ H_in = a.H_in;
    double *__restrict__ out = a.out;
    const int max_iters = a.max_iters;
    enum { DONE, STARTED, CALC_J, CHECK_ERR };
    __shared__ double red[kHomRefineThreads / 64][45];
    __shared__ double param[8], prevParam[8], JtJ[64], JtErr[8], N[64], rhs[8], dx[8];
    __shared__ double errNorm, prevErrNorm;
    __shared__ int s_wantJ, s_wantErr, s_done;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = count_ptr[0];
    int lambdaLg10 = -3, state = STARTED, iters = 0;  // thread 0's
    if (tid < 8) param[tid] = H_in[tid], prevParam[tid] = H_in[tid];
    if (tid == 0) errNorm = 0, prevErrNorm = DBL_MAX, s_done = 0;
    __syncthreads();
    for (int guard = 0; guard < 4096; ++guard) {
        if (tid == 0) {
            auto step = [&]() {
                const double lambda = exp(lambdaLg10 * 2.302585092994046);
                for (int k = 0; k < 64; ++k) N[k] = JtJ[k];
                for (int i = 0; i < 8; ++i) N[i * 8 + i] *= 1. + lambda, rhs[i] = JtErr[i];
                hom_solve8(N, rhs, dx);
                for (int i = 0; i < 8; ++i) param[i] = prevParam[i] - dx[i];
            };
            int wantJ = 0, wantErr = 0, done = 0;
            if (state == STARTED) {
                wantJ = wantErr = 1;
                state = CALC_J;
            } else if (state == CALC_J) {
                for (int i = 0; i < 8; ++i) prevParam[i] = param[i];
                step();
                prevErrNorm = errNorm;
                wantErr = 1;
                state = CHECK_ERR;
            } else {
                bool again = false;
                if (errNorm > prevErrNorm) {
                    if (++lambdaLg10 <= 16) {
                        step();
                        wantErr = 1;
                        again = true;
                    }
                }
                if (!again) {
                    lambdaLg10 = max(lambdaLg10 - 1, -16);
                    double num = 0, den = 0;
                    for (int i = 0; i < 8; ++i) num += (param[i] - prevParam[i]) * (param[i] - prevParam[i]), den += prevParam[i] * prevParam[i];
                    if (++iters >= max_iters || sqrt(num) / sqrt(den) < DBL_EPSILON) {
                        done = 1;
                    } else {
                        prevErrNorm = errNorm;
                        wantJ = 1;
                        state = CALC_J;
                    }
                }
            }
            s_wantJ = wantJ, s_wantErr = wantErr, s_done = done;
        }
        __syncthreads();
        if (s_done) break;
        const int wantJ = s_wantJ;
        double h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = param[k];
        double acc[45];
#pragma unroll
        for (int k = 0; k < 45; ++k) acc[k] = 0;
        for (int i = tid; i < count; i += kHomRefineThreads) {
            const double4 p = in_pts[i];
            double J0[8], J1[8], err[2];
            if (wantJ) hom_point_jac(h, p.x, p.y, p.z, p.w, J0, J1, err);  // (a cost-only evaluation needs no Jacobian rows)
            hom_point_err_exact(h, p.x, p.y, p.z, p.w, err);
            if (wantJ) {
                int t = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
#pragma unroll
                    for (int k = j; k < 8; ++k) acc[t++] += J0[j] * J0[k] + J1[j] * J1[k];
                    acc[36 + j] += J0[j] * err[0] + J1[j] * err[1];
                }
            }
            acc[44] += err[0] * err[0] + err[1] * err[1];
        }
#pragma unroll
        for (int k = 0; k < 45; ++k) {
            if (!wantJ && k < 44) continue;  // wave-uniform
            double v = acc[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) red[wave][k] = v;
        }
        __syncthreads();
        if (tid < 45 && (wantJ || tid == 44)) {
            double v = red[0][tid];
            for (int w = 1; w < kHomRefineThreads / 64; ++w) v += red[w][tid];
            if (tid < 36) {
                int j = 0, rem = tid;
                while (rem >= 8 - j) rem -= 8 - j, ++j;
                JtJ[j * 8 + j + rem] = v;
                JtJ[(j + rem) * 8 + j] = v;  // completeSymm
            } else if (tid < 44) {
                JtErr[tid - 36] = v;
            } else if (s_wantErr) {
                errNorm = v;
            }
        }
        __syncthreads();
    }
    if (tid < 8) out[tid] = param[tid];
    if (tid == 8) out[8] = H_in[8];
}
MLPL_HUB_KERNEL(HK_HOM_REFINE, HomRefineArgs, homog_refine_body, kHomRefineThreads);

// ------------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------------
struct HomModelHost {
    int row;                        // row of the device-side model table
    uint64_t bits[kArrFlagWords];   // inlier bits of the first flag_points correspondences
    int ext = -1;                   // index into HomogRun::ext_rows (bits of ALL correspondences) once computed
};

// The buffers of one call, sized for its largest problem (the multi-plane loop re-uses them for every plane).
// A run alone takes the blocks from the context (get); the runs of a batch get one slot each of WS_BATCH_RUNS / the batch's pinned block
// (carve), laid out for the batch's largest problem.  The blocks of the multi-plane loop follow the estimator's in the same slot.
struct HomBufs {
    char *dev = nullptr, *pin = nullptr, *pin_dev = nullptr;
    char *planes = nullptr;  // the multi-plane loop's device block (null: not wanted)
    size_t d_pts, d_H, d_ok, d_final, d_in, d_counts, dev_total;
    size_t p_smp, p_ok, p_rows, p_final, p_ext, p_ext_bytes, p_r2p, pin_total;
    // multi-plane: the label per correspondence (first: a batch clears all its slots' rows with one strided memset), the round -> plane
    // table, the round's mask, two point buffers (p1, p2, original index) the compaction alternates between
    size_t pl_labels, pl_r2p, pl_mask, pl_bufs, pl_pts_b, pl_per_buf, planes_total;
    static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }
    void layout(int n) {
        size_t o = 0;
        d_pts = o, o = up(o + (size_t)std::max(n, 1) * sizeof(double4));
        d_H = o, o = up(o + (size_t)kHomPoolSamples * 72);
        d_ok = o, o = up(o + (size_t)kHomPoolSamples * 4);
        d_final = o, o = up(o + 256);
        d_in = o, o = up(o + (size_t)std::max(n, 1) * sizeof(double4));
        d_counts = o, o = up(o + 256);
        dev_total = o + 256;
        o = 0;
        p_smp = o, o = up(o + (size_t)kHomBatchCap * kArrSmpStride * 4);
        p_ok = o, o = up(o + (size_t)kHomBatchCap * 4);
        p_rows = o, o = up(o + (size_t)kHomBatchCap * kArrFlagWords * 8);
        p_final = o, o = up(o + 256);
        p_ext_bytes = std::max((size_t)65536, (size_t)((std::max(n, 1) + 63) / 64) * 8 + 8192);  // a row list (4096 bytes) + at least one full row
        p_ext = o, o = up(o + p_ext_bytes);
        p_r2p = o, o = up(o + (size_t)std::max(n, 1) * 4 + 16);  // round -> plane (at most n / 4 rounds; padded for the 16-byte copy kernel)
        pin_total = o + 256;
        const size_t idx_b = up((size_t)std::max(n, 1) * 4 + 16);
        pl_pts_b = up((size_t)std::max(n, 1) * 16);
        pl_per_buf = 2 * pl_pts_b + idx_b;
        o = 0;
        pl_labels = o, o += idx_b;
        pl_r2p = o, o += idx_b;
        pl_mask = o, o += up((size_t)std::max(n, 1));
        pl_bufs = o, o += 2 * pl_per_buf;
        planes_total = o;
    }
    int get(mlpl_ctx *ctx, int n, bool want_planes = false) {
        layout(n);
        void *p;
        int rc;
        if ((rc = ws_get(ctx, WS_HOMOG, dev_total, &p))) return rc;
        dev = (char *)p;
        if (want_planes) {
            if ((rc = ws_get(ctx, WS_HOMOG_PLANES, planes_total, &p))) return rc;
            planes = (char *)p;
        }
        if ((rc = pinned_get(ctx, pin_total, &p))) return rc;
        pin = (char *)p;
        void *alias = nullptr;
        MLPL_HIP_TRY(hipHostGetDevicePointer(&alias, pin, 0));
        pin_dev = (char *)alias;
        return MLPL_OK;
    }
    void carve(int n_max, char *dev_slot, char *pin_slot, char *pin_dev_slot, bool want_planes) {
        layout(n_max);
        dev = dev_slot, pin = pin_slot, pin_dev = pin_dev_slot;
        planes = want_planes ? dev_slot + dev_total : nullptr;
    }
};

struct HomogRun : ArrsacTemplate<HomogRun> {  // the ARRSAC program itself: arrsac_impl.h
    mlpl_ctx *ctx;
    Launcher L;  // launches now (a run alone) or records for the hub (a run of a batch, batch_hub.h)
    const HomBufs *B;
    const double *d_p1, *d_p2;
    int n, flag_points;
    double thresh2;
    std::vector<HomModelHost> pool;
    std::vector<std::vector<uint64_t>> ext_rows;
    std::unordered_map<ArrKey, ArrIdsOf<1>, ArrKeyHash> cache;  // sample -> its model (pool index), if it gave one
    int pool_samples = 0;

    // Arrsac(4, th^2, 500, 100, 12) (pose_homography.cpp:505)
    static constexpr int kMinSample = kHomMinSample, kNonMin = kHomMaxSample, kNonMinMin = 0, kPoolSamples = kHomPoolSamples, kBatchCap = kHomBatchCap;

    int sync() { return L.sync(); }
    void pack_points() {
        HomPackArgs pa{{(n + 255) / 256, 1}, d_p1, d_p2, n, (double4 *)(B->dev + B->d_pts)};
        L.launch(HK_HOM_PACK, pa);
    }
    // the sample kernel on `keys` (checked here against n and the sample sizes): models into the table rows pool_samples ...
    int launch_samples(const std::vector<ArrKey> &keys) {
        const int nb = (int)keys.size();
        if (nb > kHomBatchCap || pool_samples + nb > kHomPoolSamples) {
            set_error("mlpl_homography_arrsac: more than %d samples solved in one call (internal capacity)", kHomPoolSamples);
            return MLPL_E_INTERNAL;
        }
        int32_t *h_smp = (int32_t *)(B->pin + B->p_smp);
        for (int b = 0; b < nb; ++b) {
            const int m = keys[b].size();
            if (m < kHomMinSample || m > kHomMaxSample) {
                set_error("mlpl_homography_arrsac: a sample of %d points (internal)", m);
                return MLPL_E_INTERNAL;
            }
            for (int i = 0; i < m; ++i)
                if (keys[b].v[1 + i] < 0 || keys[b].v[1 + i] >= n) {
                    set_error("mlpl_homography_arrsac: sample index %d outside [0, %d) (internal)", keys[b].v[1 + i], n);
                    return MLPL_E_INTERNAL;
                }
            std::memcpy(h_smp + (size_t)b * kArrSmpStride, keys[b].v, sizeof(keys[b].v));
        }
        double *d_H = (double *)(B->dev + B->d_H) + (size_t)pool_samples * 9;
        int32_t *d_ok = (int32_t *)(B->dev + B->d_ok) + pool_samples;
        HomSampleArgs sa{{nb, 1}, d_p1, d_p2, (const int32_t *)(B->pin_dev + B->p_smp), nb, d_H, d_ok};
        L.launch(HK_HOM_SAMPLE, sa);
        return MLPL_OK;
    }
    // one device batch: every key gets its cache entry
    int run_batch(const std::vector<ArrKey> &keys) {
        const int nb = (int)keys.size();
        if (nb == 0) return MLPL_OK;
        int rc;
        if ((rc = launch_samples(keys))) return rc;
        const double *d_H = (const double *)(B->dev + B->d_H) + (size_t)pool_samples * 9;
        const int32_t *d_ok = (const int32_t *)(B->dev + B->d_ok) + pool_samples;
        HomCheckArgs ca{{nb, 1}, (const double4 *)(B->dev + B->d_pts), flag_points, d_H, d_ok, nb, thresh2,
                        (unsigned long long *)(B->pin_dev + B->p_rows), (int32_t *)(B->pin_dev + B->p_ok)};
        L.launch(HK_HOM_CHECK, ca);
        if ((rc = sync())) return rc;  // kernel completion makes its system-scope writes visible
        const int32_t *h_ok = (const int32_t *)(B->pin + B->p_ok);
        const uint64_t *h_rows = (const uint64_t *)(B->pin + B->p_rows);
        for (int b = 0; b < nb; ++b) {
            ArrIdsOf<1> ids{0, {-1}};
            if (h_ok[b]) {
                HomModelHost mh;
                mh.row = pool_samples + b;
                std::memcpy(mh.bits, h_rows + (size_t)b * kArrFlagWords, sizeof(mh.bits));
                ids.id[ids.n++] = (int)pool.size();
                pool.push_back(mh);
            }
            cache.emplace(keys[b], ids);
        }
        pool_samples += nb;
        stats[8]++;
        stats[9] += nb;
        return MLPL_OK;
    }
    // Bits over all n correspondences for the given models, once each (one launch and one host hop per group that fits the mapped block).
    int ensure_ext(const std::vector<int> &ids) {
        std::vector<int> need;
        for (int id : ids)
            if (pool[id].ext == -1) {
                pool[id].ext = -2;  // queued
                need.push_back(id);
            }
        if (need.empty()) return MLPL_OK;
        const int wf = (n + 63) / 64;
        const size_t per = std::min<size_t>(1024, (B->p_ext_bytes - 4096) / ((size_t)wf * 8));  // >= 1 by the layout
        int32_t *h_rows = (int32_t *)(B->pin + B->p_ext);
        for (size_t at = 0; at < need.size(); at += per) {
            const int cnt = (int)std::min(need.size() - at, per);
            for (int i = 0; i < cnt; ++i) h_rows[i] = pool[need[at + i]].row;
            HomExtendArgs ea{{cnt, 1}, (const int32_t *)(B->pin_dev + B->p_ext), cnt, (const double4 *)(B->dev + B->d_pts), n, wf,
                             (const double *)(B->dev + B->d_H), thresh2, (unsigned long long *)(B->pin_dev + B->p_ext + 4096)};
            L.launch(HK_HOM_EXTEND, ea);
            int rc;
            if ((rc = sync())) return rc;
            const uint64_t *g = (const uint64_t *)(B->pin + B->p_ext + 4096);
            for (int i = 0; i < cnt; ++i) {
                pool[need[at + i]].ext = (int)ext_rows.size();
                ext_rows.emplace_back(g + (size_t)i * wf, g + (size_t)(i + 1) * wf);
            }
        }
        return MLPL_OK;
    }
    // The template's hook: a model arrives with its first flag_points bits; beyond them the bits of all n are computed.
    int ensure_bits(const std::vector<int> &ids, int count) { return count > flag_points ? ensure_ext(ids) : MLPL_OK; }
    bool bit(int id, int i) const {
        const HomModelHost &m = pool[id];
        if (i >= flag_points) return (ext_rows[m.ext][i >> 6] >> (i & 63)) & 1;  // callers compute the row first (ensure_bits)
        return (m.bits[i >> 6] >> (i & 63)) & 1;
    }
    void trace_turn(int, int, const ArrKey &, int, const int *) {}  // (no turn records)
};

// Where the multi-plane loop wants a plane's by-products (all device pointers, all optional).
struct HomPlaneOut {
    const int32_t *orig_in = nullptr;  // original indices of the current correspondences (null: identity)
    int32_t *label_orig = nullptr;     // per original correspondence: the round that took it as an inlier (-1 before; set by the caller)
    int label = 0;
    double *out_p1 = nullptr, *out_p2 = nullptr;
    int32_t *out_orig = nullptr;       // the outliers, compacted in order
};

// computeHomographyArrsac on device-resident correspondences.  Returns MLPL_OK (H, d_mask, *n_inliers written), MLPL_E_FAILED (the
// reference's `false`) or an error; rng_state advances whenever the estimator itself ran through.  *n_outliers (optional): what the
// compaction of HomPlaneOut holds.
static int homography_arrsac_run(mlpl_ctx *ctx, const HomBufs &B, const double *d_p1, const double *d_p2, int n, double th, uint64_t *rng_state,
                                 double *H, uint8_t *d_mask, int *n_inliers, long long *stats12, const HomPlaneOut *po, const Launcher &L) {
    if (n_inliers) *n_inliers = 0;
    if (stats12) std::memset(stats12, 0, 12 * sizeof(long long));
    if (n < 4) {
        set_error("mlpl_homography_arrsac: fewer than 4 correspondences");
        return MLPL_E_FAILED;
    }
    HomogRun R;
    R.ctx = ctx, R.L = L, R.B = &B, R.d_p1 = d_p1, R.d_p2 = d_p2, R.n = n;
    R.flag_points = std::min(n, kArrFlagPoints);
    R.thresh2 = th * th;
    int rc, row;
    if (n == 4) {  // one call of the kernel on the four correspondences, no ARRSAC; the mask is all ones
        ArrKey key;
        key.reset(0);
        for (int i = 0; i < 4; ++i) key.push(i);
        if ((rc = R.launch_samples(std::vector<ArrKey>(1, key)))) return rc;
        hub_copy_bytes(R.L, B.dev + B.d_ok, B.pin_dev + B.p_ok, 4);  // the verdict, through the mapped block
        if ((rc = R.sync())) return rc;
        const int32_t ok = *(const int32_t *)(B.pin + B.p_ok);
        if (!ok) {
            set_error("mlpl_homography_arrsac: the four correspondences are degenerate");
            return MLPL_E_FAILED;
        }
        row = 0;
    } else {
        R.prosac_rng.state = rng_state[0], R.random_rng.state = rng_state[1];
        R.pack_points();
        rc = MLPL_OK;
        const int best = R.estimate(&rc);
        if (stats12) std::memcpy(stats12, R.stats, sizeof(R.stats));
        if (rc) return rc;  // an internal limit or a HIP error is not an estimator outcome: the caller's stream states stay where they were
        rng_state[0] = R.prosac_rng.state, rng_state[1] = R.random_rng.state;
        if (best < 0) {
            set_error("mlpl_homography_arrsac: no hypothesis passed the sequential test");
            return MLPL_E_FAILED;
        }
        row = R.pool[best].row;
    }
    // findHomographyInliers with the winner, refineHomography on its inliers (n > 4 only); the refined matrix, the winner and the counts
    // come back through the mapped block
    const double *d_Hbest = (const double *)(B.dev + B.d_H) + (size_t)row * 9;
    double *h_final = (double *)(B.pin + B.p_final), *h_final_dev = (double *)(B.pin_dev + B.p_final);
    int32_t *h_counts = (int32_t *)(h_final + 18), *h_counts_dev = (int32_t *)(h_final_dev + 18);
    int32_t *d_counts = (int32_t *)(B.dev + B.d_counts);
    double4 *d_in = (double4 *)(B.dev + B.d_in);
    HomInliersArgs ia{{1, 1}, d_p1, d_p2, n, d_Hbest, th * th, n == 4 ? 1 : 0, d_mask, po ? po->orig_in : nullptr, po ? po->label_orig : nullptr,
                      po ? po->label : 0, d_in, po ? po->out_p1 : nullptr, po ? po->out_p2 : nullptr, po ? po->out_orig : nullptr, d_counts};
    R.L.launch(HK_HOM_INLIERS, ia);
    if (n != 4) {
        HomRefineArgs ra{{1, 1}, (const double4 *)d_in, (const int32_t *)d_counts, d_Hbest, 10, h_final_dev};
        R.L.launch(HK_HOM_REFINE, ra);
    }
    HomFinalArgs fa{{1, 1}, d_Hbest, (const int32_t *)d_counts, h_final_dev + 9, h_counts_dev};
    R.L.launch(HK_HOM_FINAL, fa);
    if ((rc = R.sync())) return rc;
    std::memcpy(H, n == 4 ? h_final + 9 : h_final, 72);
    if (n_inliers) *n_inliers = h_counts[0];
    if (stats12) stats12[11] = h_counts[1];
    return MLPL_OK;
}

}  // namespace

int homography_arrsac_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double th, uint64_t *rng_state, double *H, uint8_t *d_mask,
                          int *n_inliers, long long *stats12, hipStream_t s) {
    HomBufs B;
    int rc;
    if ((rc = B.get(ctx, n))) return rc;
    Launcher L;
    L.s = s;
    return homography_arrsac_run(ctx, B, d_p1, d_p2, n, th, rng_state, H, d_mask, n_inliers, stats12, nullptr, L);
}

// findHomographyInliers alone: d_mask (n bytes) and the count
int homography_inliers_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const double *H, double th, uint8_t *d_mask, int *n_inliers,
                           hipStream_t s) {
    HomBufs B;
    int rc;
    if ((rc = B.get(ctx, n))) return rc;
    double *h_final = (double *)(B.pin + B.p_final);
    std::memcpy(h_final, H, 72);
    int32_t *d_counts = (int32_t *)(B.dev + B.d_counts);
    HomInliersArgs ia{{1, 1}, d_p1, d_p2, n, (const double *)(B.pin_dev + B.p_final), th * th, 0, d_mask, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                      nullptr, d_counts};
    hub_kernels()[HK_HOM_INLIERS].single(&ia, s);
    MLPL_HIP_TRY(hipGetLastError());
    int32_t cnt[2] = {0, 0};
    MLPL_HIP_TRY(hipMemcpyAsync(cnt, d_counts, 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    if (n_inliers) *n_inliers = cnt[0];
    return MLPL_OK;
}

// The sample kernel on `count` index lists of m points each (host), for tests: H [count][9], ok [count]
int homography_sample_models(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const int32_t *idx, int m, int count, double *H, int32_t *ok,
                             hipStream_t s) {
    HomBufs B;
    int rc;
    if ((rc = B.get(ctx, n))) return rc;
    HomogRun R;
    R.ctx = ctx, R.L.s = s, R.B = &B, R.d_p1 = d_p1, R.d_p2 = d_p2, R.n = n;
    std::vector<ArrKey> keys((size_t)count);
    for (int b = 0; b < count; ++b) {
        keys[b].reset(HomogRun::sample_kind(m));
        for (int i = 0; i < m; ++i) keys[b].push(idx[(size_t)b * m + i]);
    }
    if ((rc = R.launch_samples(keys))) return rc == MLPL_E_INTERNAL ? MLPL_E_BAD_INPUT : rc;
    MLPL_HIP_TRY(hipGetLastError());
    MLPL_HIP_TRY(hipMemcpyAsync(H, B.dev + B.d_H, (size_t)count * 72, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(ok, B.dev + B.d_ok, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    return MLPL_OK;
}

// The planes of the multi-plane loop for the caller: label_round[j] = the round that took correspondence j (-1 none), round_to_plane[r] =
// the output index of that round's plane (-1: not reported).  labels_out[j] (optional) = output plane or -1; masks (optional) = n_planes
// rows of n flags.
namespace {
struct HomPlanesOutArgs {  // 256 threads per block
    KHdr hdr;
    const int32_t *label_round;
    int n;
    const int32_t *round_to_plane;
    int n_planes;
    int32_t *labels_out;
    uint8_t *masks;
};
__device__ __forceinline__ void homog_planes_out_body(const HomPlanesOutArgs &a, int bx, int) {
    const int32_t *__restrict__ label_round = a.label_round, *__restrict__ round_to_plane = a.round_to_plane;
    int32_t *__restrict__ labels_out = a.labels_out;
    uint8_t *__restrict__ masks = a.masks;
    const int n = a.n, n_planes = a.n_planes;
    const int j = bx * 256 + threadIdx.x;
    if (j >= n) return;
    const int r = label_round[j];
    const int k = r >= 0 ? round_to_plane[r] : -1;
    if (labels_out) labels_out[j] = k;
    if (masks)
        for (int p = 0; p < n_planes; ++p) masks[(size_t)p * n + j] = k == p ? 1 : 0;
}
MLPL_HUB_KERNEL(HK_HOM_PLANES_OUT, HomPlanesOutArgs, homog_planes_out_body, 256);

// estimateMultHomographys (pose_homography.cpp:291-463): plane after plane, the outliers of one round are the next round's input in
// their original order; the correspondences stay on the device between planes (two buffers the compaction alternates between).  The
// planes' inlier sets are disjoint, so the device keeps ONE label per correspondence (the round that took it) however many planes are
// found.  Per plane only H and the counts come back; the masks (d_masks: device, cap * n bytes, original indexing) and / or the labels
// (d_labels: device, n int32, output plane index or -1) are written at the end, if asked for.  Outputs in the reference's order: by inlier
// count, descending (std::sort on the reference's pairs) when more than one plane was found; found_at[k] (optional) = the round that found
// output plane k (ascending found_at = the order of discovery).  *n_planes = -1: no homography found (the reference's return value -1).
// Finding more than cap planes is MLPL_E_BAD_INPUT with rng_state put back, so the call can be repeated with larger arrays.
// B holds the blocks of the loop (HomBufs::planes); a run of a batch (L.hub set) finds its label row cleared by the batch driver.
static int mult_homographies_run(mlpl_ctx *ctx, const HomBufs &B, const double *d_p1, const double *d_p2, int n, double th, int var_th, unsigned max_planes,
                                 unsigned min_pts, uint64_t *rng_state, int cap, int *n_planes, double *Hs, int32_t *num_inl, double *strength,
                                 double *th_used, uint8_t *d_masks, int32_t *d_labels, int32_t *found_at, Launcher L) {
    *n_planes = 0;
    const uint64_t rng_in[2] = {rng_state[0], rng_state[1]};
    int rc;
    const size_t pts_b = B.pl_pts_b, per_buf = B.pl_per_buf;
    const bool want_labels = d_masks || d_labels;
    char *w = B.planes + B.pl_bufs;
    uint8_t *d_round_mask = (uint8_t *)(B.planes + B.pl_mask);
    int32_t *d_label_round = (int32_t *)(B.planes + B.pl_labels), *d_round_to_plane = (int32_t *)(B.planes + B.pl_r2p);
    if (want_labels && !L.hub) MLPL_HIP_TRY(hipMemsetAsync(d_label_round, 0xFF, (size_t)n * 4, L.s));
    struct Plane {
        double H[9], strength, th_used;
        unsigned n_inl;
        int round;
    };
    std::vector<Plane> planes;
    const double *cur_p1 = d_p1, *cur_p2 = d_p2;
    const int32_t *cur_orig = nullptr;
    unsigned n_inl = (unsigned)n, n_rest = (unsigned)n, i = 0;
    int nc = n;
    const double maxTh = th * 6.0, th_mult = 1.5, th_mult_base = 1.5;
    // (i < n: a round that takes no correspondence at all -- possible only with minPtsPerPlane = 0 -- would never end; the tables hold n rounds)
    while (n_rest > 3 && n_inl >= min_pts && (!max_planes || i < max_planes) && i < (unsigned)n) {
        char *nb = w + (size_t)(i & 1) * per_buf;
        HomPlaneOut po;
        po.orig_in = cur_orig;
        po.out_p1 = (double *)nb, po.out_p2 = (double *)(nb + pts_b), po.out_orig = (int32_t *)(nb + 2 * pts_b);
        if (want_labels) po.label_orig = d_label_round, po.label = (int)i;
        double th_tmp = th * th_mult_base, H[9];
        int cnt = 0;
        do {
            rc = homography_arrsac_run(ctx, B, cur_p1, cur_p2, nc, th_tmp, rng_state, H, d_round_mask, &cnt, nullptr, &po, L);
            if (rc && rc != MLPL_E_FAILED) return rc;
            th_tmp *= th_mult;
        } while (var_th && rc == MLPL_E_FAILED && th_tmp < maxTh);
        if (rc == MLPL_E_FAILED) {
            if (!i) {
                *n_planes = -1;
                return MLPL_OK;
            }
            break;
        }
        n_inl = (unsigned)cnt;
        n_rest -= n_inl;
        if (n_inl >= min_pts) {
            if ((int)planes.size() >= cap) {
                rng_state[0] = rng_in[0], rng_state[1] = rng_in[1];
                set_error("mlpl_mult_homographies: more than cap = %d planes found (the stream states were put back)", cap);
                return MLPL_E_BAD_INPUT;
            }
            Plane pl;
            std::memcpy(pl.H, H, 72);
            pl.n_inl = n_inl;
            pl.th_used = th_tmp / th_mult;
            pl.strength = th * th_mult_base * (double)n_inl / (pl.th_used * (double)n);
            pl.round = (int)i;
            planes.push_back(pl);
        }
        cur_p1 = po.out_p1, cur_p2 = po.out_p2, cur_orig = po.out_orig;
        nc = (int)n_rest;
        i++;
    }
    std::vector<std::pair<unsigned, unsigned>> order;
    for (unsigned k = 0; k < planes.size(); ++k) order.push_back(std::make_pair(k, planes[k].n_inl));
    if (planes.size() > 1)
        std::sort(order.begin(), order.end(), [](std::pair<unsigned, unsigned> const &a, std::pair<unsigned, unsigned> const &b) { return a.second > b.second; });
    // i rounds ran (every round took at least 4 correspondences: i <= n / 4); the table is built in the run's mapped block
    int32_t *round_to_plane = (int32_t *)(B.pin + B.p_r2p);
    const size_t n_rounds = (size_t)std::max(i, 1u);
    for (size_t r = 0; r < n_rounds; ++r) round_to_plane[r] = -1;
    for (size_t k = 0; k < planes.size(); ++k) {
        const Plane &pl = planes[order[k].first];
        std::memcpy(Hs + 9 * k, pl.H, 72);
        num_inl[k] = (int32_t)pl.n_inl, strength[k] = pl.strength, th_used[k] = pl.th_used;
        if (found_at) found_at[k] = pl.round;
        round_to_plane[(size_t)pl.round] = (int32_t)k;
    }
    if (want_labels && !planes.empty()) {
        hub_copy_bytes(L, B.pin_dev + B.p_r2p, d_round_to_plane, n_rounds * 4);
        HomPlanesOutArgs oa{{(n + 255) / 256, 1}, (const int32_t *)d_label_round, n, (const int32_t *)d_round_to_plane, (int)planes.size(), d_labels, d_masks};
        L.launch(HK_HOM_PLANES_OUT, oa);
        if ((rc = L.sync())) return rc;  // the mapped block is the next call's
    }
    *n_planes = (int)planes.size();
    return MLPL_OK;
}
}  // namespace

int mult_homographies_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double th, int var_th, unsigned max_planes, unsigned min_pts,
                          uint64_t *rng_state, int cap, int *n_planes, double *Hs, int32_t *num_inl, double *strength, double *th_used, uint8_t *d_masks,
                          int32_t *d_labels, int32_t *found_at, hipStream_t s) {
    HomBufs B;
    int rc;
    if ((rc = B.get(ctx, n, true))) return rc;
    Launcher L;
    L.s = s;
    return mult_homographies_run(ctx, B, d_p1, d_p2, n, th, var_th, max_planes, min_pts, rng_state, cap, n_planes, Hs, num_inl, strength, th_used, d_masks,
                                 d_labels, found_at, L);
}

// ---- batches of plane problems on the hub's cohort / lane driver (batch_hub.h hub_batch_drive) -----------------------------------------------------
// A run's slot is a HomBufs laid out for the batch's largest problem.  job(b, bufs, launcher) is problem b's sequential program -- the one
// the single entries run -- and returns its status.  Every problem's outputs are those of the single entry on it alone.
namespace {
constexpr int kHomBatchRuns = 128;

static int homography_batch_drive(mlpl_ctx *ctx, int B, const int32_t *counts, bool want_planes, bool clear_labels, int32_t *status, hipStream_t s,
                                  const char *name, const std::function<int(int, const HomBufs &, const Launcher &)> &job) {
    int n_max = 1;
    for (int b = 0; b < B; ++b) n_max = std::max(n_max, counts[b]);
    HomBufs Y;
    Y.layout(n_max);
    const size_t slot_dev = Y.dev_total + (want_planes ? HomBufs::up(Y.planes_total) : 0);
    HubBatch P{name, kHomBatchRuns, slot_dev, Y.pin_total, true, nullptr};
    if (clear_labels)  // the label rows of all the cohort's slots: -1 = taken by no round
        P.before_cohort = [=](const HubCohort &c) {
            if (hipMemset2DAsync(c.dev + Y.dev_total + Y.pl_labels, slot_dev, 0xFF, (size_t)n_max * 4, (size_t)c.size, c.stream) == hipSuccess) return (int)MLPL_OK;
            set_error("%s: clearing the label rows failed", name);
            return (int)MLPL_E_HIP;
        };
    HubBatchStats st;
    const int rc = hub_batch_drive(ctx, B, P, status, s, [&](int b, const HubSlot &slot, const Launcher &L) {
        HomBufs bufs;
        bufs.carve(n_max, slot.dev, slot.pin, slot.pin_dev, want_planes);
        return job(b, bufs, L);
    }, st);
    hub_arrsac_stats(ctx, st);
    return rc;
}
}  // namespace

int homography_arrsac_batch_dev(mlpl_ctx *ctx, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double th,
                                uint64_t *rng_states, double *H, uint8_t *d_masks, int32_t *n_inliers, int32_t *status, long long *stats, hipStream_t s) {
    return homography_batch_drive(ctx, B, counts, false, false, status, s, "mlpl_homography_arrsac_batch_dev", [&](int b, const HomBufs &Bf, const Launcher &L) {
        int ninl = 0;  // (fewer than 4 correspondences: MLPL_E_FAILED before anything is touched)
        const int r = homography_arrsac_run(ctx, Bf, d_p1 + (size_t)b * stride * 2, d_p2 + (size_t)b * stride * 2, counts[b], th, rng_states + 2 * (size_t)b,
                                            H + (size_t)b * 9, d_masks + (size_t)b * stride, &ninl, stats ? stats + (size_t)b * 12 : nullptr, nullptr, L);
        if (n_inliers) n_inliers[b] = ninl;
        return r;
    });
}

int mult_homographies_batch_dev(mlpl_ctx *ctx, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double th, int var_th,
                                unsigned max_planes, unsigned min_pts, uint64_t *rng_states, int cap, int32_t *n_planes, double *Hs, int32_t *num_inl,
                                double *strength, double *th_used, int32_t *found_at, int32_t *d_labels, int32_t *status, hipStream_t s) {
    return homography_batch_drive(ctx, B, counts, true, d_labels != nullptr, status, s, "mlpl_mult_homographies_batch_dev",
                                  [&](int b, const HomBufs &Bf, const Launcher &L) {
        if (counts[b] < 4) {
            n_planes[b] = -1;
            return (int)MLPL_E_FAILED;
        }
        const size_t at = (size_t)b * cap;
        int np = 0;
        const int r = mult_homographies_run(ctx, Bf, d_p1 + (size_t)b * stride * 2, d_p2 + (size_t)b * stride * 2, counts[b], th, var_th, max_planes, min_pts,
                                            rng_states + 2 * (size_t)b, cap, &np, Hs + at * 9, num_inl + at, strength + at, th_used + at, nullptr,
                                            d_labels ? d_labels + (size_t)b * stride : nullptr, found_at ? found_at + at : nullptr, L);
        n_planes[b] = np;
        return r;
    });
}

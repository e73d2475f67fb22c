// homography_oracle.cpp -- a sequential restatement of poselib's computeHomographyArrsac / estimateMultHomographys for the tests:
// theia::Arrsac<size_t, cv::Mat>(4, th^2, 500, 100, 12) around the normalised 4-point DLT, cv::findHomography(m1, m2, 0) for the
// non-minimal samples, findHomographyInliers and refineHomography (CvLevMarq).  One hypothesis at a time, float64, plain loops, a cyclic
// Jacobi instead of cv::eigen, its own cv::RNG.  cv::eigen, LMSolver::run and CvLevMarq::updateAlt / step are restated from memory of
// OpenCV 4.x; this file is NOT pinned against a build of the reference or of OpenCV -- the device code is pinned against this file.
// The hypothesis lists are re-ordered with libstdc++'s std::sort, as the reference does and as the library does: ties are the norm.
//
// variant = 1 walks the Jacobi pairs in reverse order and adds the LtL / JtJ sums from the last point to the first: the yardstick for
// how far two correct evaluations of the same formulas may differ.
// margin: the minimum over every threshold comparison made of |sqrt(err) - th| / th.
// doubt (ho_last_refine_doubt): the largest relative size |param - prevParam| / |prevParam| of a step that refineHomography REJECTED.
// CvLevMarq accepts a step iff the cost did not rise.  The last Gauss-Newton steps that still matter (~1e-10 of H) change the cost by
// less than the rounding of its own sum, so in plain doubles that test is a coin flip: a run of rejections raises lambda until the step
// vanishes, the relative-change test fires and H stays short of the fixed point.  Two correct evaluations then differ by the size of the
// rejected step although they agree on every other decision; a scene whose doubt exceeds the tolerance cannot pin H.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Rng {  // cv::RNG: multiply-with-carry
    uint64_t state;
    unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
        return (unsigned)state;
    }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

struct Problem {
    const double *p1, *p2;  // n x 2 each
    int n;
    int variant;
    double margin;
    double doubt = 0.0;
};
double g_last_doubt = 0.0;

// symmetric eigenproblem, cyclic Jacobi; w: eigenvalues, V[k][*]: eigenvector k (rows), sorted descending as cv::eigen returns them
void eigen_sym(int n, const double *A_in, double *w, double *V, int variant) {
    std::vector<double> A(A_in, A_in + n * n), U(n * n, 0.0);
    for (int i = 0; i < n; ++i) U[i * n + i] = 1.0;
    std::vector<std::pair<int, int>> pairs;
    for (int p = 0; p < n; ++p)
        for (int q = p + 1; q < n; ++q) pairs.push_back({p, q});
    if (variant) std::reverse(pairs.begin(), pairs.end());
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0, diag = 0;
        for (int p = 0; p < n; ++p) {
            diag += A[p * n + p] * A[p * n + p];
            for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
        }
        if (!(off > 1e-34 * diag)) break;
        for (auto pq : pairs) {
            const int p = pq.first, q = pq.second;
            const double apq = A[p * n + q];
            if (apq == 0.0) continue;
            const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
            double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
            if (theta < 0) t = -t;
            const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < n; ++k) {  // columns p, q
                const double akp = A[k * n + p], akq = A[k * n + q];
                A[k * n + p] = c * akp - s * akq;
                A[k * n + q] = s * akp + c * akq;
            }
            for (int k = 0; k < n; ++k) {  // rows p, q
                const double apk = A[p * n + k], aqk = A[q * n + k];
                A[p * n + k] = c * apk - s * aqk;
                A[q * n + k] = s * apk + c * aqk;
            }
            for (int k = 0; k < n; ++k) {
                const double ukp = U[k * n + p], ukq = U[k * n + q];
                U[k * n + p] = c * ukp - s * ukq;
                U[k * n + q] = s * ukp + c * ukq;
            }
        }
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[a * n + a] > A[b * n + b]; });
    for (int k = 0; k < n; ++k) {
        w[k] = A[order[k] * n + order[k]];
        for (int r = 0; r < n; ++r) V[k * n + r] = U[r * n + order[k]];
    }
}

void mat3_mul(const double *a, const double *b, double *c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
            c[i * 3 + j] = s;
        }
}

// runHomogrophyKernel: M -> m, count points (x, y pairs)
bool dlt_kernel(const double *M, const double *m, int count, double *H, int variant) {
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = 0; i < count; ++i) {
        cmx += m[2 * i], cmy += m[2 * i + 1];
        cMx += M[2 * i], cMy += M[2 * i + 1];
    }
    cmx /= count, cmy /= count, cMx /= count, cMy /= count;
    for (int i = 0; i < count; ++i) {
        smx += std::fabs(m[2 * i] - cmx), smy += std::fabs(m[2 * i + 1] - cmy);
        sMx += std::fabs(M[2 * i] - cMx), sMy += std::fabs(M[2 * i + 1] - cMy);
    }
    if (std::fabs(smx) < DBL_EPSILON || std::fabs(smy) < DBL_EPSILON || std::fabs(sMx) < DBL_EPSILON || std::fabs(sMy) < DBL_EPSILON) return false;
    smx = count / smx, smy = count / smy, sMx = count / sMx, sMy = count / sMy;
    const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
    const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    double LtL[81];
    for (int k = 0; k < 81; ++k) LtL[k] = 0;
    for (int ii = 0; ii < count; ++ii) {
        const int i = variant ? count - 1 - ii : ii;
        const double x = (m[2 * i] - cmx) * smx, y = (m[2 * i + 1] - cmy) * smy;
        const double X = (M[2 * i] - cMx) * sMx, Y = (M[2 * i + 1] - cMy) * sMy;
        const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
        const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
        for (int j = 0; j < 9; ++j)
            for (int k = j; k < 9; ++k) LtL[j * 9 + k] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
    }
    for (int j = 0; j < 9; ++j)
        for (int k = 0; k < j; ++k) LtL[j * 9 + k] = LtL[k * 9 + j];
    double W[9], V[81];
    eigen_sym(9, LtL, W, V, variant);
    double Htemp[9], H0[9];
    mat3_mul(invHnorm, V + 72, Htemp);
    mat3_mul(Htemp, Hnorm2, H0);
    const double inv = 1. / H0[8];
    for (int k = 0; k < 9; ++k) H[k] = H0[k] * inv;
    return true;
}

// 8 x 8 linear system by Gaussian elimination with partial pivoting (OpenCV's DECOMP_EIG / DECOMP_SVD are not restated)
void solve8(const double *A_in, const double *b_in, double *x) {
    double A[64], b[8];
    std::memcpy(A, A_in, sizeof(A));
    std::memcpy(b, b_in, sizeof(b));
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        for (int r = c + 1; r < 8; ++r)
            if (std::fabs(A[r * 8 + c]) > std::fabs(A[piv * 8 + c])) piv = r;
        if (piv != c) {
            for (int k = 0; k < 8; ++k) std::swap(A[c * 8 + k], A[piv * 8 + k]);
            std::swap(b[c], b[piv]);
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

// residuals and, when JtJ != null, J^T J (full, symmetric) and J^T r of the transfer error over `count` points
void homography_sums(const double *M, const double *m, int count, const double *h, double *JtJ, double *JtErr, double *errNorm, double *rinf, int variant) {
    if (JtJ) {
        for (int k = 0; k < 64; ++k) JtJ[k] = 0;
        for (int k = 0; k < 8; ++k) JtErr[k] = 0;
    }
    double en = 0, ri = 0;
    for (int ii = 0; ii < count; ++ii) {
        const int i = variant ? count - 1 - ii : ii;
        const double Mx = M[2 * i], My = M[2 * i + 1];
        double ww = h[6] * Mx + h[7] * My + 1.;
        ww = std::fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
        const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
        const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
        const double err[2] = {xi - m[2 * i], yi - m[2 * i + 1]};
        if (JtJ) {
            const double J[2][8] = {{Mx * ww, My * ww, ww, 0, 0, 0, -Mx * ww * xi, -My * ww * xi}, {0, 0, 0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi}};
            for (int j = 0; j < 8; ++j) {
                for (int k = j; k < 8; ++k) JtJ[j * 8 + k] += J[0][j] * J[0][k] + J[1][j] * J[1][k];
                JtErr[j] += J[0][j] * err[0] + J[1][j] * err[1];
            }
        }
        en += err[0] * err[0] + err[1] * err[1];
        if (std::fabs(err[0]) > ri) ri = std::fabs(err[0]);
        if (std::fabs(err[1]) > ri) ri = std::fabs(err[1]);
    }
    if (JtJ)
        for (int j = 0; j < 8; ++j)
            for (int k = 0; k < j; ++k) JtJ[j * 8 + k] = JtJ[k * 8 + j];
    if (errNorm) *errNorm = en;
    if (rinf) *rinf = ri;
}

// LMSolver::run (OpenCV 4.x calib3d levmarq.cpp) on the 8 parameters, maxIters turns, epsx = epsf = FLT_EPSILON
void lm_polish(const double *M, const double *m, int count, double *h, int maxIters, int variant) {
    double x[8], xd[8], A[64], v[8], D[8], Ap[64], d[8], S, rinf;
    std::memcpy(x, h, sizeof(x));
    homography_sums(M, m, count, x, A, v, &S, &rinf, variant);
    for (int i = 0; i < 8; ++i) D[i] = A[i * 8 + i];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        std::memcpy(Ap, A, sizeof(A));
        for (int i = 0; i < 8; ++i) Ap[i * 8 + i] += lambda * D[i];
        solve8(Ap, v, d);
        for (int i = 0; i < 8; ++i) xd[i] = x[i] - d[i];
        double Sd;
        homography_sums(M, m, count, xd, nullptr, nullptr, &Sd, nullptr, variant);
        double dS = 0, t = 0;
        for (int i = 0; i < 8; ++i) {
            double td = 2 * v[i];
            for (int k = 0; k < 8; ++k) td -= A[i * 8 + k] * d[k];
            dS += d[i] * td;
            t += d[i] * v[i];
        }
        const double R = (S - Sd) / (std::fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double nu = (Sd - S) / (std::fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = std::min(std::max(nu, 2.), 10.);
            if (lambda == 0) {
                double maxval = DBL_EPSILON;
                for (int c = 0; c < 8; ++c) {  // diagonal of A^-1
                    double e[8] = {0, 0, 0, 0, 0, 0, 0, 0}, col[8];
                    e[c] = 1;
                    solve8(A, e, col);
                    maxval = std::max(maxval, std::fabs(col[c]));
                }
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
            std::memcpy(x, xd, sizeof(x));
            homography_sums(M, m, count, x, A, v, &S, &rinf, variant);
        }
        iter++;
        double dinf = 0;
        for (int i = 0; i < 8; ++i)
            if (std::fabs(d[i]) > dinf) dinf = std::fabs(d[i]);
        const bool proceed = iter < maxIters && dinf >= (double)FLT_EPSILON && rinf >= (double)FLT_EPSILON;
        if (!proceed) break;
    }
    std::memcpy(h, x, sizeof(x));
}

// cv::findHomography(m1, m2, 0) on float32-rounded points + the reference's rejection
bool nonminimal_model(const double *M, const double *m, int count, double *H, int variant, int polish) {
    std::vector<double> Mf(2 * count), mf(2 * count);
    for (int k = 0; k < 2 * count; ++k) Mf[k] = (double)(float)M[k], mf[k] = (double)(float)m[k];
    if (!dlt_kernel(Mf.data(), mf.data(), count, H, variant)) return false;
    if (polish) lm_polish(Mf.data(), mf.data(), count, H, 10, variant);
    if (H[0] == 0.0 || H[8] == 0.0) return false;
    return true;
}

// refineHomography: CvLevMarq(8, 0, {maxIters, DBL_EPSILON}) driven through updateAlt
void refine_homography(const double *M, const double *m, int count, double *H, int maxIters, int variant, double *doubt = nullptr) {
    enum { DONE, STARTED, CALC_J, CHECK_ERR };
    double param[8], prevParam[8], JtJ[64], JtErr[8], errNorm = 0, prevErrNorm = DBL_MAX;
    int lambdaLg10 = -3, state = STARTED, iters = 0;
    std::memcpy(param, H, sizeof(param));
    auto step = [&]() {
        const double lambda = std::exp(lambdaLg10 * std::log(10.));
        double N[64], dx[8];
        std::memcpy(N, JtJ, sizeof(N));
        for (int i = 0; i < 8; ++i) N[i * 8 + i] *= 1. + lambda;
        solve8(N, JtErr, dx);
        for (int i = 0; i < 8; ++i) param[i] = prevParam[i] - dx[i];
    };
    for (;;) {
        bool wantJ = false, wantErr = false;
        if (state == DONE) break;
        if (state == STARTED) {
            wantJ = wantErr = true;
            state = CALC_J;
        } else if (state == CALC_J) {
            std::memcpy(prevParam, param, sizeof(param));
            step();
            prevErrNorm = errNorm;
            wantErr = true;
            state = CHECK_ERR;
        } else {
            bool again = false;
            if (errNorm > prevErrNorm) {
                if (doubt) {
                    double num = 0, den = 0;
                    for (int i = 0; i < 8; ++i) num += (param[i] - prevParam[i]) * (param[i] - prevParam[i]), den += prevParam[i] * prevParam[i];
                    *doubt = std::max(*doubt, std::sqrt(num) / std::sqrt(den));
                }
                if (++lambdaLg10 <= 16) {
                    step();
                    wantErr = true;
                    state = CHECK_ERR;
                    again = true;
                }
            }
            if (!again) {
                lambdaLg10 = std::max(lambdaLg10 - 1, -16);
                double num = 0, den = 0;
                for (int i = 0; i < 8; ++i) num += (param[i] - prevParam[i]) * (param[i] - prevParam[i]), den += prevParam[i] * prevParam[i];
                if (++iters >= maxIters || std::sqrt(num) / std::sqrt(den) < DBL_EPSILON) {
                    state = DONE;
                    break;
                }
                prevErrNorm = errNorm;
                wantJ = true;
                state = CALC_J;
            }
        }
        double en;
        homography_sums(M, m, count, param, wantJ ? JtJ : nullptr, wantJ ? JtErr : nullptr, &en, nullptr, variant);
        if (wantErr) errNorm = en;
    }
    std::memcpy(H, param, sizeof(param));
}

struct Scored {
    int id;
    double score;
};

struct Arrsac {
    Problem &P;
    double th, thresh2;
    Rng prosac_rng, random_rng;
    static constexpr int kMinSample = 4, kMaxHyps = 500, kBlock = 100, kNonMin = 12, kNonMinMin = 0, kMaxInner = 20;
    static constexpr double kConf = 0.95, kTimeRatio = 250.0;
    double sigma = 0.05, epsilon = 0.1;
    int verified_accum = 0, num_rejected = 0;
    double rejected_accum = 0.0;
    long long stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> models;  // 9 doubles each

    double error(int i, const double *H) const {
        const double Mx = P.p1[2 * i], My = P.p1[2 * i + 1], mx = P.p2[2 * i], my = P.p2[2 * i + 1];
        const double ww = 1. / (H[6] * Mx + H[7] * My + 1.);
        const double dx = (H[0] * Mx + H[1] * My + H[2]) * ww - mx;
        const double dy = (H[3] * Mx + H[4] * My + H[5]) * ww - my;
        return dx * dx + dy * dy;
    }
    void note(double err) {
        if (std::isfinite(err)) P.margin = std::min(P.margin, std::fabs(std::sqrt(err) - th) / th);
    }
    bool inlier(int i, int id) {
        const double e = error(i, &models[(size_t)id * 9]);
        note(e);
        return e < thresh2;
    }
    // one model per sample: returns its id or -1
    int estimate(const std::vector<int> &s, bool minimal) {
        std::vector<double> M(2 * s.size()), m(2 * s.size());
        for (size_t k = 0; k < s.size(); ++k) {
            M[2 * k] = P.p1[2 * s[k]], M[2 * k + 1] = P.p1[2 * s[k] + 1];
            m[2 * k] = P.p2[2 * s[k]], m[2 * k + 1] = P.p2[2 * s[k] + 1];
        }
        double H[9];
        const bool ok = minimal ? dlt_kernel(M.data(), m.data(), (int)s.size(), H, P.variant) : nonminimal_model(M.data(), m.data(), (int)s.size(), H, P.variant, 1);
        if (!ok) return -1;
        models.insert(models.end(), H, H + 9);
        return (int)(models.size() / 9) - 1;
    }
    static int to_int_x86(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }
    static int hyps_needed(double eps, double power) {
        return std::min(kMaxHyps, to_int_x86(std::ceil(std::log(1.0 - kConf) / std::log(1.0 - std::pow(eps, power)))));
    }
    static double sprt_threshold(double sg, double ep, int nmv) {
        const double c = (1.0 - sg) * std::log((1.0 - sg) / (1.0 - ep)) + sg * std::log(sg / ep);
        const double a_0 = kTimeRatio * c / static_cast<double>(nmv) + 1.0;
        double t = a_0;
        for (int i = 0; i < 1000; i++) {
            const double nt = a_0 + std::log(t);
            const double step = std::fabs(nt - t);
            t = nt;
            if (step < 1e-4) break;
        }
        return t;
    }
    bool sprt(int id, int count, double dt, double *ratio, int *num_inl) {
        *num_inl = 0;
        double lr = 1.0;
        for (int i = 0; i < count; ++i) {
            if (inlier(i, id)) {
                lr *= sigma / epsilon;
                *num_inl += 1;
            } else {
                lr *= (1.0 - sigma) / (1.0 - epsilon);
            }
            if (lr > dt) {
                *ratio = static_cast<double>(*num_inl) / static_cast<double>(i + 1);
                return false;
            }
        }
        *ratio = static_cast<double>(*num_inl) / static_cast<double>(count);
        return true;
    }
    void rejected(double ratio) {
        rejected_accum += ratio;
        num_rejected++;
        const double st = rejected_accum / static_cast<double>(num_rejected);
        if (st > 0) sigma = st;
    }
    void prosac_sample(int count, int k, std::vector<int> &s) {  // ProsacSampler::Sample, sample number k
        double t_n = 200000;
        int nn = kMinSample;
        for (int i = 0; i < kMinSample; i++) t_n *= static_cast<double>(nn - i) / (double)((size_t)count - i);
        double t_n_prime = 1.0;
        for (int t = 1; t <= k; t++) {
            if (t > t_n_prime && nn < count) {
                const double t_n_plus1 = (t_n * ((double)nn + 1.0)) / ((double)nn + 1.0 - (double)kMinSample);
                t_n_prime += std::ceil(t_n_plus1 - t_n);
                t_n = t_n_plus1;
                nn++;
            }
        }
        s.clear();
        auto has = [&](int r) { return std::find(s.begin(), s.end(), r) != s.end(); };
        if (t_n_prime < k) {
            for (int i = 0; i < kMinSample; i++) {
                int r;
                do r = prosac_rng.uniform(0, nn);
                while (has(r));
                s.push_back(r);
            }
        } else {
            for (int i = 0; i < kMinSample - 1; i++) {
                int r;
                do r = prosac_rng.uniform(0, nn - 1);
                while (has(r));
                s.push_back(r);
            }
            s.push_back(nn - 1);
        }
    }
    void random_sample(const std::vector<int> &universe, int size, std::vector<int> &s) {
        std::vector<int> used;
        s.clear();
        for (int i = 0; i < size; i++) {
            int r;
            do r = random_rng.uniform(0, (int)universe.size());
            while (std::find(used.begin(), used.end(), r) != used.end());
            used.push_back(r);
            s.push_back(universe[r]);
        }
    }

    int initial_set(int count, std::vector<Scored> &accepted) {
        int k = 1, k2 = 0, m_prime = kMaxHyps, inner_its = 0, max_num_inliers = 0, random_size = kNonMin;
        bool inner = false;
        std::vector<int> data, s;
        while (k <= m_prime) {
            int id;
            if (!inner) {
                prosac_sample(count, k, s);
                stats[2]++;
                id = estimate(s, true);
            } else {
                random_sample(data, random_size, s);
                stats[3]++;
                id = estimate(s, random_size == kMinSample || random_size < kNonMinMin);
                inner_its++;
                if (inner_its == kMaxInner) inner_its = 0, inner = false;
            }
            if (id < 0) {
                k2++, k++;
                continue;
            }
            verified_accum += 1;
            const double dt = sprt_threshold(sigma, epsilon, verified_accum / (k - k2));
            int num_inl;
            double ratio;
            if (!sprt(id, count, dt, &ratio, &num_inl)) {
                rejected(ratio);
            } else if (num_inl > max_num_inliers) {
                max_num_inliers = num_inl;
                accepted.push_back(Scored{id, (double)num_inl});
                if (num_inl > kMinSample) {
                    inner = true;
                    inner_its = 0;
                    random_size = std::max(std::min(kNonMin, (int)std::floor((float)max_num_inliers / 2.0f)), kMinSample);
                    data.clear();
                    for (int i = 0; i < count; i++)
                        if (inlier(i, id)) data.push_back(i);
                    epsilon = ratio == 1.0 ? 0.9999 : ratio;
                    m_prime = hyps_needed(epsilon, (double)kMinSample);
                    stats[4]++;
                }
            } else {
                accepted.push_back(Scored{id, (double)num_inl});
            }
            k++;
        }
        if (accepted.empty()) return 0;
        return k - k2 - 1;
    }

    int run() {  // Arrsac::Estimate: id of the best model or -1
        const int n = P.n;
        const int sub_block = (int)std::floor((float)kBlock / 5.0);
        const int kill_thresh = (int)std::floor(7.0 * (float)sub_block / 12.0);
        std::vector<Scored> hyps;
        int k = initial_set(std::min(n, kBlock), hyps);
        stats[0] = k, stats[1] = (long long)hyps.size();
        if (k == 0) return -1;
        if (n <= kBlock) {
            double hi = 0.0;
            int at = 0;
            for (size_t i = 0; i < hyps.size(); i++)
                if (hyps[i].score > hi) hi = hyps[i].score, at = (int)i;
            return hyps[at].id;
        }
        auto cmp = [](Scored a, Scored b) { return a.score > b.score; };
        std::vector<int> all(n), s;
        for (int i = 0; i < n; ++i) all[i] = i;
        int nh = (int)hyps.size();
        int i = kBlock;
        for (; i < n; i++) {
            if ((i + 1) % kBlock == 0) {
                std::sort(hyps.begin(), hyps.end(), cmp);
                double max_inliers = hyps[0].score;
                epsilon = max_inliers / static_cast<double>(i + 1);
                if (epsilon == 1.0) epsilon = 0.9999;
                int temp_max = hyps_needed(epsilon, (double)(i + 1));
                if (temp_max > k) {
                    int k2 = 0;
                    for (int j = 0; j < (long long)temp_max - k; j++) {
                        random_sample(all, kMinSample, s);
                        stats[5]++;
                        const int id = estimate(s, true);
                        if (id < 0) {
                            k2++;
                            continue;
                        }
                        verified_accum += 1;
                        const double dt = sprt_threshold(sigma, epsilon, verified_accum / (k + j + 1 - k2));
                        int num_inl;
                        double ratio;
                        if (!sprt(id, i + 1, dt, &ratio, &num_inl)) {
                            rejected(ratio);
                        } else if (num_inl > (int)max_inliers) {
                            hyps.push_back(Scored{id, (double)num_inl});
                            max_inliers = static_cast<double>(num_inl);
                            epsilon = ratio == 1.0 ? 0.9999 : ratio;
                            temp_max = hyps_needed(epsilon, (double)(i + 1));
                            // (one model per sample: the reference's `break` out of the model loop ends nothing else)
                        } else {
                            hyps.push_back(Scored{id, (double)num_inl});
                        }
                        k++;
                    }
                    nh = (int)hyps.size();
                } else {
                    const int n1 = std::max(1, (int)std::floor((float)k * std::pow(2.0, -1.0 * std::floor((float)(i + 1) / (float)kBlock))));
                    if (n1 < static_cast<int>(hyps.size())) {
                        hyps.resize(n1);
                        nh = n1;
                    }
                }
            } else if ((i + 1) % sub_block == 0) {
                std::sort(hyps.begin(), hyps.end(), cmp);
                int j = nh - 1;
                for (; j > 0; j--)
                    if (hyps[j - 1].score - hyps[j].score > kill_thresh) break;
                nh = nh - j;
                hyps.resize(nh);
            }
            if (nh == 1) break;
            for (size_t j = 0; j < hyps.size(); j++)
                if (inlier(i, hyps[j].id)) hyps[j].score += 1.0;
        }
        stats[6] = i, stats[7] = nh;
        return hyps[0].id;
    }
};

// computeHomographyArrsac; returns 1 / 0
int homography_arrsac(Problem &P, double th, uint64_t *rng, double *H, uint8_t *mask, int *n_inliers, long long *stats8) {
    const int n = P.n;
    if (stats8) std::memset(stats8, 0, 8 * sizeof(long long));
    if (n_inliers) *n_inliers = 0;
    if (n < 4) return 0;
    if (n == 4) {
        if (!dlt_kernel(P.p1, P.p2, 4, H, P.variant)) return 0;
        if (mask) std::memset(mask, 1, 4);
        if (n_inliers) *n_inliers = 4;
        return 1;
    }
    Arrsac A{P, th, th * th, Rng{rng[0]}, Rng{rng[1]}};
    const int best = A.run();
    rng[0] = A.prosac_rng.state, rng[1] = A.random_rng.state;
    if (stats8) std::memcpy(stats8, A.stats, sizeof(A.stats));
    if (best < 0) return 0;
    std::memcpy(H, &A.models[(size_t)best * 9], 72);
    std::vector<double> M, m;
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        const double e = A.error(i, H);
        A.note(e);
        const bool in = !(e > th * th);
        if (mask) mask[i] = in ? 1 : 0;
        if (in) {
            M.push_back(P.p1[2 * i]), M.push_back(P.p1[2 * i + 1]);
            m.push_back(P.p2[2 * i]), m.push_back(P.p2[2 * i + 1]);
            cnt++;
        }
    }
    if (n_inliers) *n_inliers = cnt;
    refine_homography(M.data(), m.data(), cnt, H, 10, P.variant, &P.doubt);
    return 1;
}

}  // namespace

extern "C" {

double ho_last_refine_doubt() { return g_last_doubt; }  // of the last ho_homography_arrsac / ho_mult_homographies call (largest over its planes)

int ho_homography_arrsac(const double *p1, const double *p2, int n, double th, uint64_t *rng, int variant, double *H, uint8_t *mask,
                         int *n_inliers, long long *stats8, double *margin) {
    Problem P{p1, p2, n, variant, HUGE_VAL};
    const int ok = homography_arrsac(P, th, rng, H, mask, n_inliers, stats8);
    if (margin) *margin = P.margin;
    g_last_doubt = P.doubt;
    return ok;
}

// the model of one sample: m == 4 the minimal kernel, m > 4 findHomography(., ., 0) (polish = 0: without its LM turns) and the rejection
int ho_sample_model(const double *p1, const double *p2, const int32_t *idx, int m, int variant, int polish, double *H) {
    std::vector<double> M(2 * m), mm(2 * m);
    for (int k = 0; k < m; ++k) {
        M[2 * k] = p1[2 * idx[k]], M[2 * k + 1] = p1[2 * idx[k] + 1];
        mm[2 * k] = p2[2 * idx[k]], mm[2 * k + 1] = p2[2 * idx[k] + 1];
    }
    for (int k = 0; k < 9; ++k) H[k] = 0;
    return (m == 4 ? dlt_kernel(M.data(), mm.data(), m, H, variant) : nonminimal_model(M.data(), mm.data(), m, H, variant, polish)) ? 1 : 0;
}

int ho_homography_inliers(const double *p1, const double *p2, int n, const double *H, double th, uint8_t *mask) {
    Problem P{p1, p2, n, 0, HUGE_VAL};
    Arrsac A{P, th, th * th, Rng{0}, Rng{0}};
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        const bool in = !(A.error(i, H) > th * th);
        mask[i] = in ? 1 : 0;
        cnt += in;
    }
    return cnt;
}

// estimateMultHomographys; returns 0 / -1.  Planes in the reference's output order (sorted by inlier count when more than one was found);
// masks in the original indexing, cap * n bytes (or null).
int ho_mult_homographies(const double *p1, const double *p2, int n, double th, int var_th, unsigned max_planes, unsigned min_pts, uint64_t *rng,
                         int variant, int cap, int *n_planes, double *Hs, int *num_inl, double *strength, double *th_used, uint8_t *masks,
                         double *margin) {
    *n_planes = 0;
    g_last_doubt = 0.0;
    if (margin) *margin = HUGE_VAL;
    if (n <= 3) return -1;
    std::vector<double> q1(p1, p1 + 2 * n), q2(p2, p2 + 2 * n);
    std::vector<int> orig(n);
    for (int i = 0; i < n; ++i) orig[i] = i;
    struct Plane {
        double H[9], strength, th_used;
        unsigned n_inl;
        std::vector<uint8_t> mask;
    };
    std::vector<Plane> planes;
    unsigned n_inl = (unsigned)n, n_rest = (unsigned)n, i = 0;
    const double maxTh = th * 6.0, th_mult = 1.5, th_mult_base = 1.5;
    while (n_rest > 3 && n_inl >= min_pts && (!max_planes || i < max_planes)) {
        const int nc = (int)orig.size();
        double th_tmp = th * th_mult_base, H[9];
        std::vector<uint8_t> mask(nc);
        int ok, cnt = 0;
        do {
            Problem P{q1.data(), q2.data(), nc, variant, HUGE_VAL};
            ok = homography_arrsac(P, th_tmp, rng, H, mask.data(), &cnt, nullptr);
            if (margin) *margin = std::min(*margin, P.margin);
            g_last_doubt = std::max(g_last_doubt, P.doubt);
            th_tmp *= th_mult;
        } while (var_th && !ok && th_tmp < maxTh);
        if (!ok) {
            if (!i) return -1;
            break;
        }
        n_inl = (unsigned)cnt;
        n_rest -= n_inl;
        if (n_inl >= min_pts) {
            Plane pl;
            std::memcpy(pl.H, H, 72);
            pl.n_inl = n_inl;
            pl.th_used = th_tmp / th_mult;
            pl.strength = th * th_mult_base * (double)n_inl / (pl.th_used * (double)n);
            pl.mask.assign(n, 0);
            for (int j = 0; j < nc; ++j)
                if (mask[j]) pl.mask[orig[j]] = 1;
            planes.push_back(pl);
        }
        std::vector<double> r1, r2;
        std::vector<int> ro;
        for (int j = 0; j < nc; ++j)
            if (!mask[j]) {
                r1.push_back(q1[2 * j]), r1.push_back(q1[2 * j + 1]);
                r2.push_back(q2[2 * j]), r2.push_back(q2[2 * j + 1]);
                ro.push_back(orig[j]);
            }
        q1.swap(r1), q2.swap(r2), orig.swap(ro);
        i++;
    }
    std::vector<std::pair<unsigned, unsigned>> order;
    for (unsigned k = 0; k < planes.size(); ++k) order.push_back({k, planes[k].n_inl});
    if (planes.size() > 1)
        std::sort(order.begin(), order.end(), [](std::pair<unsigned, unsigned> const &a, std::pair<unsigned, unsigned> const &b) { return a.second > b.second; });
    *n_planes = (int)planes.size();
    for (int k = 0; k < (int)planes.size() && k < cap; ++k) {
        const Plane &pl = planes[order[k].first];
        std::memcpy(Hs + 9 * k, pl.H, 72);
        num_inl[k] = (int)pl.n_inl, strength[k] = pl.strength, th_used[k] = pl.th_used;
        if (masks) std::memcpy(masks + (size_t)k * n, pl.mask.data(), n);
    }
    return 0;
}
}

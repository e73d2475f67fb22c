// homography_align_oracle.cpp -- sequential fp64 restatement of the pose-from-planes half of poselib::estimatePoseHomographies:
// Homographys_Alignment (poselib/source/HomographyAlignment.cpp:197-360) with Longuet_Higgins_Solution[_with_initial], jacobi_mat_33,
// Check_motion_error, update_dn, update_h0_rt (the equilibrated LU with implicit pivoting), check_error, then the caller's part
// (ComputeHomographyMotion :82-171 and pose_homography.cpp:195-213).  Written anew from the algorithm; plain g++, no dependencies.
// Built as libhomography_align_oracle.so by csrc/facade/Makefile (or by tests/homography_align_oracle.py when it is missing).
//
// Two variants of the same arithmetic: variant 0 adds every sum in the reference's order (plane after plane, a plane's points in index
// order) and sweeps the Jacobi pairs (0,1) (0,2) (1,2); variant 1 adds from the last plane / last point to the first and sweeps the pairs
// backwards.  Their difference is the yardstick S_A of tests/homography_pose_scenes.py.
//
// Restated from memory of OpenCV (not readable next to the reference): a 3 x 3 Mat::inv() is the cofactor formula times 1 / det and the
// ZERO matrix when det == 0; determinant() of a 3 x 3 is the first-row expansion; Mat / scalar multiplies by 1. / scalar; a small matrix
// product adds over k in ascending order; cv::norm of a 3-vector is sqrt(x^2 + y^2 + z^2) added in that order.
//
// Where the reference's behaviour is not defined the restatement returns -3 ("Homography alignment failed") with a reason word:
//   1  a Longuet-Higgins decomposition refuses H (not d0 > 1 && d2 <= 1; the reference ignores the return value)
//   2  fewer than two of its four sign candidates have plane(2) > 0 (the reference indexes the second one regardless)
//   3  Check_motion_error counted no point (the reference divides by zero)
//   4  a result is not finite
//   5  fewer than two planes (defined in the reference: ComputeHomographyMotion returns 0 because t1_2 is empty)
//   6  a plane without correspondences (the reference's caller never passes one: a plane holds at least 15)
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

typedef double M3[3][3];

struct Run {
    const double *p1, *p2;
    std::vector<std::vector<int>> idx;  // idx[k]: the correspondences of plane k in summation order
    std::vector<int> plane_order;       // planes in summation order
    int P = 0, variant = 0;
    double margin_stop = INFINITY;  // closest stop-test comparison (relative)
    int fail = 0;
};

void mul33(const M3 a, const M3 b, M3 c) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += a[i][k] * b[k][j];
            r[i][j] = s;
        }
    std::memcpy(c, r, sizeof(M3));
}
void mulv(const M3 a, const double *x, double *y) {
    double r[3];
    for (int i = 0; i < 3; ++i) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += a[i][k] * x[k];
        r[i] = s;
    }
    y[0] = r[0], y[1] = r[1], y[2] = r[2];
}
void mulTv(const M3 a, const double *x, double *y) {  // a^T x
    double r[3];
    for (int i = 0; i < 3; ++i) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += a[k][i] * x[k];
        r[i] = s;
    }
    y[0] = r[0], y[1] = r[1], y[2] = r[2];
}
double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
double norm3(const double *a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
double det33(const M3 m) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
void inv33(const M3 s, M3 out) {  // zero matrix when singular
    double d = det33(s);
    M3 t;
    if (d != 0.) {
        d = 1. / d;
        t[0][0] = (s[1][1] * s[2][2] - s[1][2] * s[2][1]) * d;
        t[0][1] = (s[0][2] * s[2][1] - s[0][1] * s[2][2]) * d;
        t[0][2] = (s[0][1] * s[1][2] - s[0][2] * s[1][1]) * d;
        t[1][0] = (s[1][2] * s[2][0] - s[1][0] * s[2][2]) * d;
        t[1][1] = (s[0][0] * s[2][2] - s[0][2] * s[2][0]) * d;
        t[1][2] = (s[0][2] * s[1][0] - s[0][0] * s[1][2]) * d;
        t[2][0] = (s[1][0] * s[2][1] - s[1][1] * s[2][0]) * d;
        t[2][1] = (s[0][1] * s[2][0] - s[0][0] * s[2][1]) * d;
        t[2][2] = (s[0][0] * s[1][1] - s[0][1] * s[1][0]) * d;
    } else {
        std::memset(t, 0, sizeof(M3));
    }
    std::memcpy(out, t, sizeof(M3));
}

// Cyclic Jacobi on a symmetric 3 x 3 (at most 50 sweeps, off-diagonal sum below 1e-6 ends it); eigenvalues sorted descending by three
// neighbour swaps, the columns of v following.  Returns 0 when the sweeps ran out (d, v as they stand, unsorted), as the reference does.
void rot_pair(M3 a, int i, int j, int k, int l, double s, double tau) {
    const double g = a[i][j], h = a[k][l];
    a[i][j] = g - s * (h + g * tau);
    a[k][l] = h + s * (g - h * tau);
}
void swap_cols(M3 v, int c0, int c1) {
    for (int r = 0; r < 3; ++r) {
        const double t = v[r][c0];
        v[r][c0] = v[r][c1], v[r][c1] = t;
    }
}
int jacobi33(const M3 a_in, double *d, M3 v, int variant) {
    M3 a;
    std::memcpy(a, a_in, sizeof(M3));
    double b[3], z[3];
    for (int p = 0; p < 3; ++p) {
        for (int q = 0; q < 3; ++q) v[p][q] = 0.0;
        v[p][p] = 1.0;
        b[p] = d[p] = a[p][p];
        z[p] = 0.0;
    }
    static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sweep = 1; sweep <= 50; ++sweep) {
        double sm = 0.0;
        for (int k = 0; k < 3; ++k) {
            const int *pq = pairs[variant ? 2 - k : k];
            sm += std::fabs(a[pq[0]][pq[1]]);
        }
        if (sm < 0.000001) {
            if (d[1] > d[0]) { const double c = d[0]; d[0] = d[1], d[1] = c; swap_cols(v, 0, 1); }
            if (d[2] > d[1]) { const double c = d[1]; d[1] = d[2], d[2] = c; swap_cols(v, 1, 2); }
            if (d[1] > d[0]) { const double c = d[0]; d[0] = d[1], d[1] = c; swap_cols(v, 0, 1); }
            return 1;
        }
        const double tresh = sweep < 4 ? 0.2 * sm / 9 : 0.0;
        for (int k = 0; k < 3; ++k) {
            const int ip = pairs[variant ? 2 - k : k][0], iq = pairs[variant ? 2 - k : k][1];
            const double g = 100.0 * std::fabs(a[ip][iq]);
            if (sweep > 4 && (std::fabs(d[ip]) + g) == std::fabs(d[ip]) && (std::fabs(d[iq]) + g) == std::fabs(d[iq])) {
                a[ip][iq] = 0.0;
            } else if (std::fabs(a[ip][iq]) > tresh) {
                double h = d[iq] - d[ip], t;
                if ((std::fabs(h) + g) == std::fabs(h)) {
                    t = a[ip][iq] / h;
                } else {
                    const double theta = 0.5 * h / a[ip][iq];
                    t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(1 + t * t), s = t * c, tau = s / (1.0 + c);
                h = t * a[ip][iq];
                z[ip] -= h, z[iq] += h, d[ip] -= h, d[iq] += h;
                a[ip][iq] = 0.0;
                for (int j = 0; j <= ip - 1; ++j) rot_pair(a, j, ip, j, iq, s, tau);
                for (int j = ip + 1; j <= iq - 1; ++j) rot_pair(a, ip, j, j, iq, s, tau);
                for (int j = iq + 1; j < 3; ++j) rot_pair(a, ip, j, iq, j, s, tau);
                for (int j = 0; j < 3; ++j) rot_pair(v, j, ip, j, iq, s, tau);
            }
        }
        for (int p = 0; p < 3; ++p) b[p] += z[p], d[p] = b[p], z[p] = 0.0;
    }
    return 0;
}

// The two-view decomposition of a plane homography (Longuet-Higgins 1981 / Cheng 2010).  n_cand candidates (R, t, n) with n(2) > 0.
// Returns 1, 2 for "degenerate to a rotation" (both candidates R = H / sqrt(d1), t = n = 0), 0 for refused.
struct Decomp {
    M3 R[2];
    double t[2][3], n[2][3];
    int n_cand;
};
int decompose(const M3 H, Decomp &D, int variant) {
    M3 W, u, hn;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += H[k][i] * H[k][j];
            W[i][j] = s;
        }
    double d[3];
    jacobi33(W, d, u, variant);
    const double d2 = 1.0 / std::sqrt(d[1]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) hn[i][j] = d2 * H[i][j];
    d[0] = d[0] / d[1], d[2] = d[2] / d[1], d[1] = 1.0;
    D.n_cand = 0;
    if (d[0] - d[1] < 0.000001 && d[1] - d[2] < 0.000001) {
        for (int c = 0; c < 2; ++c) {
            std::memcpy(D.R[c], hn, sizeof(M3));
            for (int j = 0; j < 3; ++j) D.t[c][j] = 0, D.n[c][j] = 0;
        }
        D.n_cand = 2;
        return 2;
    }
    if (!(d[0] > 1.0 && d[2] <= 1.0)) return 0;
    const double den = d[0] - d[2];
    const double t0 = std::sqrt((d[0] - 1.0) * d[2] / den), t2 = std::sqrt((1.0 - d[2]) * d[0] / den);
    const double q0 = std::sqrt((d[0] - 1.0) * d[0] / den), q2 = std::sqrt((1.0 - d[2]) * d[2] / den);
    for (int s1 = -1; s1 <= 1; s1 += 2)
        for (int s2 = -1; s2 <= 1; s2 += 2) {
            const double ps0 = -s1 * q0, ps2 = -s2 * q2;
            const double nv[3] = {s1 * t0 + ps0, 0.0, s2 * t2 + ps2}, ts[3] = {s1 * t0, 0.0, s2 * t2};
            double trans[3], plane[3];
            mulv(u, ts, trans);
            mulv(u, nv, plane);
            if (plane[2] > 0.0) {
                if (D.n_cand < 2) {
                    std::memcpy(D.t[D.n_cand], trans, 24);
                    std::memcpy(D.n[D.n_cand], plane, 24);
                }
                ++D.n_cand;
            }
        }
    if (D.n_cand > 2) D.n_cand = 2;  // (cannot happen: the candidates come in pairs of opposite planes)
    for (int c = 0; c < D.n_cand; ++c) {
        M3 tn, inv;
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) tn[j][k] = D.t[c][j] * D.n[c][k];
        tn[0][0] -= 1.0, tn[1][1] -= 1.0, tn[2][2] -= 1.0;
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) tn[j][k] = -1.0 * tn[j][k];
        inv33(tn, inv);
        mul33(hn, inv, D.R[c]);
        if (det33(D.R[c]) < 0.0)
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k) D.R[c][j][k] = -1.0 * D.R[c][j][k];
    }
    return 1;
}

template <class F>
void for_points(const Run &r, int k, F f) {
    for (int i : r.idx[k]) f(i);
}

// mean distance between the closest points of the two viewing rays of every correspondence under (R, t); -1 when no ray pair counted
double motion_error(const Run &r, const M3 R, const double *t) {
    double error = 0;
    long total = 0;
    for (int k : r.plane_order) {
        double e1 = 0;
        for_points(r, k, [&](int i) {
            const double a[3] = {r.p1[2 * i], r.p1[2 * i + 1], 1.0}, b[3] = {r.p2[2 * i], r.p2[2 * i + 1], 1.0};
            const double ia = 1. / norm3(a);
            const double r1[3] = {a[0] * ia, a[1] * ia, a[2] * ia};
            double pb[3];
            mulTv(R, b, pb);
            const double ib = 1. / norm3(pb);
            const double r2[3] = {pb[0] * ib, pb[1] * ib, pb[2] * ib};
            const double dotp = dot3(r1, r2);
            if (std::fabs(dotp) > 0.9999999) return;
            const double bv1 = dot3(t, r1), bv2 = dot3(t, r2);
            double m1, m2;
            if (dotp == 0.0) {
                m1 = bv1, m2 = bv2;
            } else {
                m1 = (bv1 - bv2 * dotp) / (1.0 - dotp * dotp);
                m2 = dotp * m1 - bv2;
            }
            const double dp[3] = {m1 * r1[0] - (t[0] + m2 * r2[0]), m1 * r1[1] - (t[1] + m2 * r2[1]), m1 * r1[2] - (t[2] + m2 * r2[2])};
            e1 += norm3(dp);
            ++total;
        });
        error += e1;
    }
    if (total == 0) return -1.0;
    return error / (double)total;
}

void update_dn(const Run &r, int k, const double *h, const double *k0, double *dn) {
    M3 A = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, inv;
    double B[3] = {0, 0, 0};
    for_points(r, k, [&](int i) {
        const double p[3] = {r.p1[2 * i], r.p1[2 * i + 1], 1.0}, x2 = r.p2[2 * i], y2 = r.p2[2 * i + 1];
        double hp[3];
        for (int j = 0; j < 3; ++j) hp[j] = h[3 * j] * p[0] + h[3 * j + 1] * p[1] + h[3 * j + 2] * p[2];
        for (int row = 0; row < 2; ++row) {
            const double m = row ? y2 : x2, d = k0[2] * m;
            double t[3];
            for (int j = 0; j < 3; ++j) t[j] = k0[row] * p[j] - d * p[j];
            const double y = m * hp[2] - hp[row];
            for (int j = 0; j < 3; ++j) {
                for (int l = 0; l < 3; ++l) A[j][l] = t[j] * t[l] + A[j][l];
                B[j] = y * t[j] + B[j];
            }
        }
    });
    inv33(A, inv);
    mulv(inv, B, dn);
}

// LU of the TRANSPOSE of a (n x n, row-major) with row equilibration and implicit pivoting; ps = the pivot sequence.  0 = singular.
int lu_decompose(const double *a, double *lu, int *ps, int n) {
    double scales[32];
    for (int i = 0; i < n; ++i) {
        double biggest = 0.0;
        for (int j = 0; j < n; ++j) {
            const double v = std::fabs(lu[i * n + j] = a[j * n + i]);
            if (biggest < v) biggest = v;
        }
        if (biggest == 0.0) return 0;
        scales[i] = 1.0 / biggest;
        ps[i] = i;
    }
    for (int k = 0; k < n - 1; ++k) {
        double biggest = 0.0;
        int pivotindex = k;
        for (int i = k; i < n; ++i) {
            const double v = std::fabs(lu[ps[i] * n + k]) * scales[ps[i]];
            if (biggest < v) biggest = v, pivotindex = i;
        }
        if (biggest == 0.0) return 0;
        if (pivotindex != k) {
            const int j = ps[k];
            ps[k] = ps[pivotindex], ps[pivotindex] = j;
        }
        const double pivot = lu[ps[k] * n + k];
        for (int i = k + 1; i < n; ++i) {
            const double mult = lu[ps[i] * n + k] = lu[ps[i] * n + k] / pivot;
            if (mult != 0.0)
                for (int j = k + 1; j < n; ++j) lu[ps[i] * n + j] -= mult * lu[ps[k] * n + j];
        }
    }
    return lu[ps[n - 1] * n + n - 1] != 0.0;
}
void lu_solve(const double *lu, const int *ps, const double *b, double *x, int n) {
    for (int i = 0; i < n; ++i) {
        double dot = 0.0;
        for (int j = 0; j < i; ++j) dot += lu[ps[i] * n + j] * x[j];
        x[i] = b[ps[i]] - dot;
    }
    for (int i = n - 1; i >= 0; --i) {
        double dot = 0.0;
        for (int j = i + 1; j < n; ++j) dot += lu[ps[i] * n + j] * x[j];
        x[i] = (x[i] - dot) / lu[ps[i] * n + i];
    }
}
// m = inverse(a) b the reference's way: row i of the inverse is the solve for unit vector i, then m_i = sum_j inv_ij b_j.  0 = singular.
int solve_by_inverse(const double *a, const double *b, double *m, int n) {
    double lu[32 * 32], x[32], e[32];
    int ps[32];
    if (!lu_decompose(a, lu, ps, n)) return 0;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) e[j] = 0;
        e[i] = 1;
        lu_solve(lu, ps, e, x, n);
        double s = 0;
        for (int j = 0; j < n; ++j) s += x[j] * b[j];
        m[i] = s;
    }
    return 1;
}

// the 11 unknowns (h0..h7, rt) from all planes at once; a singular system leaves h and rt as they were
int update_h0_rt(const Run &r, double *h, const double *dn, double *rt) {
    double a[121], b[11], m[11];
    for (int i = 0; i < 121; ++i) a[i] = 0;
    for (int i = 0; i < 11; ++i) b[i] = 0;
    for (int k : r.plane_order)
        for_points(r, k, [&](int i) {
            const double x1 = r.p1[2 * i], y1 = r.p1[2 * i + 1], x2 = r.p2[2 * i], y2 = r.p2[2 * i + 1];
            const double dnp = x1 * dn[3 * k] + y1 * dn[3 * k + 1] + 1.0 * dn[3 * k + 2];
            const double rx[11] = {x1, y1, 1.0, 0, 0, 0, -x1 * x2, -y1 * x2, dnp, 0, -x2 * dnp};
            const double ry[11] = {0, 0, 0, x1, y1, 1.0, -x1 * y2, -y1 * y2, 0, dnp, -y2 * dnp};
            for (int row = 0; row < 2; ++row) {
                const double *rr = row ? ry : rx, d = row ? y2 : x2;
                for (int j = 0; j < 11; ++j) {
                    for (int l = 0; l < 11; ++l) a[j * 11 + l] = rr[j] * rr[l] + a[j * 11 + l];
                    b[j] = d * rr[j] + b[j];
                }
            }
        });
    if (!solve_by_inverse(a, b, m, 11)) return 0;
    for (int j = 0; j < 8; ++j) h[j] = m[j];
    h[8] = 1.0;
    rt[0] = m[8], rt[1] = m[9], rt[2] = m[10];
    return 1;
}

double transfer_error(const Run &r, const double *h0, const double *dn, const double *rt) {
    double error = 0;
    long total = 0;
    for (int k : r.plane_order) {
        double h[9];
        for (int j = 0; j < 3; ++j)
            for (int l = 0; l < 3; ++l) h[3 * j + l] = h0[3 * j + l] + rt[j] * dn[3 * k + l];
        const double s = 1.0 / h[8];
        for (int j = 0; j < 9; ++j) h[j] = s * h[j];
        double e1 = 0;
        for_points(r, k, [&](int i) {
            const double x = r.p1[2 * i], y = r.p1[2 * i + 1];
            const double w0 = h[0] * x + h[1] * y + h[2] * 1.0, w1 = h[3] * x + h[4] * y + h[5] * 1.0, w2 = h[6] * x + h[7] * y + h[8] * 1.0;
            const double dx = w0 / w2 - r.p2[2 * i], dy = w1 / w2 - r.p2[2 * i + 1];
            e1 += std::sqrt(dx * dx + dy * dy);
            ++total;
        });
        error += e1;
    }
    return error / (float)total;
}

void note_stop(Run &r, double e1, double e2, double c, double tol) {
    const double m1 = std::fabs(std::fabs(e1 - e2) - c) / c, m2 = std::fabs(e1 - tol) / tol;
    if (m1 < r.margin_stop) r.margin_stop = m1;
    if (m2 < r.margin_stop) r.margin_stop = m2;
}

bool finite_all(const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

// info (24 doubles): [0] code (0 / -3), [1] chosen q, [2..5] rounds per outer turn for q = 0 (0 = turn not run), [6..9] for q = 1,
// [10] [11] last e1 per q, [12..15] motion errors (the two initial candidates, the two results), [16] candidate choices (bit 4 q + turn
// set when the second sign candidate was taken), [17] reason of a -3 (see the head of this file), [18] closest stop-test margin
// (relative), [19] relative distance of the two final motion errors.  Outputs are written only when the code is 0.
extern "C" int hao_alignment(const double *p1, const double *p2, const int32_t *labels, int n, int P, const double *H0, double tol, int variant,
                             double *R_out, double *t_out, double *E_out, double *norms_out, double *Hs_out, double *info) {
    for (int i = 0; i < 24; ++i) info[i] = 0;
    auto fail = [&](int reason) {
        info[0] = -3, info[17] = reason;
        return -3;
    };
    if (P < 2) return fail(5);
    Run r;
    r.p1 = p1, r.p2 = p2, r.P = P, r.variant = variant;
    r.idx.resize((size_t)P);
    for (int i = 0; i < n; ++i)
        if (labels[i] >= 0 && labels[i] < P) r.idx[(size_t)labels[i]].push_back(i);
    for (int k = 0; k < P; ++k) {
        if (r.idx[(size_t)k].empty()) return fail(6);
        r.plane_order.push_back(variant ? P - 1 - k : k);
    }
    if (variant)
        for (auto &v : r.idx) v = std::vector<int>(v.rbegin(), v.rend());

    M3 Hm;
    std::memcpy(Hm, H0, sizeof(M3));
    Decomp D0;
    const int d0 = decompose(Hm, D0, variant);
    if (d0 == 0) return fail(1);
    if (D0.n_cand < 2) return fail(2);
    double errors[2];
    for (int c = 0; c < 2; ++c) {
        errors[c] = motion_error(r, D0.R[c], D0.t[c]);
        if (errors[c] < 0) return fail(3);
        info[12 + c] = errors[c];
    }
    std::vector<double> dn((size_t)3 * P, 0.0), dn_q0((size_t)3 * P, 0.0);
    M3 rotq[2];
    double tq[2][3], nq[2][3];
    int choice_bits = 0;
    for (int q = 0; q < 2; ++q) {
        double h0[9], rt0[3], dt_b[3], norm_b[3] = {0, 0, 0};
        M3 rot_b;
        std::memcpy(h0, H0, 72);
        mulv(D0.R[q], D0.t[q], rt0);
        std::memcpy(rot_b, D0.R[q], sizeof(M3));
        std::memcpy(dt_b, D0.t[q], 24);
        double e1 = 0, e2 = 100000.0;
        for (int turn = 0; turn < 4; ++turn) {
            int iter;
            for (iter = 0; iter < 40; ++iter) {
                dn[0] = dn[1] = dn[2] = 0;
                for (int k = 1; k < P; ++k) update_dn(r, k, h0, rt0, &dn[3 * (size_t)k]);
                update_h0_rt(r, h0, dn.data(), rt0);
                e1 = transfer_error(r, h0, dn.data(), rt0);
                if (iter > 2) note_stop(r, e1, e2, 0.00001, tol);
                if ((std::fabs(e1 - e2) < 0.00001 || e1 < tol) && iter > 2) break;
                e2 = e1;
            }
            info[2 + 4 * q + turn] = iter < 40 ? iter + 1 : 40;
            M3 h0m;
            std::memcpy(h0m, h0, 72);
            Decomp D;
            const int dr = decompose(h0m, D, variant);
            if (dr == 0) return fail(1);
            if (D.n_cand < 2) return fail(2);
            const int pick = dr == 2 ? 0 : (dot3(D.t[0], dt_b) > dot3(D.t[1], dt_b) ? 0 : 1);
            if (pick) choice_bits |= 1 << (4 * q + turn);
            std::memcpy(dt_b, D.t[pick], 24);
            std::memcpy(norm_b, D.n[pick], 24);
            std::memcpy(rot_b, D.R[pick], sizeof(M3));
            mulv(rot_b, dt_b, rt0);
            e1 = transfer_error(r, h0, dn.data(), rt0);
            if (iter > 2) note_stop(r, e1, e2, 0.000001, tol);
            if ((std::fabs(e1 - e2) < 0.000001 || e1 < tol) && iter > 2) break;
            e2 = e1;
        }
        std::memcpy(rotq[q], rot_b, sizeof(M3));
        std::memcpy(tq[q], dt_b, 24);
        std::memcpy(nq[q], norm_b, 24);
        info[10 + q] = e1;
        if (q == 0) dn_q0 = dn;
    }
    info[16] = choice_bits;
    for (int q = 0; q < 2; ++q) {
        errors[q] = motion_error(r, rotq[q], tq[q]);
        if (errors[q] < 0) return fail(3);
        info[14 + q] = errors[q];
    }
    const int q = errors[0] < errors[1] ? 0 : 1;
    info[1] = q;
    info[18] = r.margin_stop;
    {
        const double big = std::fmax(std::fabs(errors[0]), std::fabs(errors[1]));
        info[19] = big > 0 ? std::fabs(errors[0] - errors[1]) / big : 0.0;
    }
    const double *t12 = tq[q], *n0 = nq[q];
    M3 hh, RI;
    for (int j = 0; j < 3; ++j)
        for (int l = 0; l < 3; ++l) hh[j][l] = (j == l ? 1.0 : 0.0) - t12[j] * n0[l];
    mul33(rotq[q], hh, RI);
    const double s1 = RI[2][2];
    // (the reference takes the plane offsets of the FIRST candidate's run whichever q it chose: dn2.rowRange(0, num_patches))
    std::vector<double> norms((size_t)3 * P), Hs((size_t)9 * P);
    for (int l = 0; l < 3; ++l) norms[l] = n0[l];
    for (int k = 1; k < P; ++k)
        for (int l = 0; l < 3; ++l) norms[3 * k + l] = n0[l] - s1 * dn_q0[3 * k + l];
    for (int k = 0; k < P; ++k) {
        M3 tp, h;
        for (int j = 0; j < 3; ++j)
            for (int l = 0; l < 3; ++l) tp[j][l] = (j == l ? 1.0 : 0.0) - t12[j] * norms[3 * k + l];
        mul33(rotq[q], tp, h);
        if (std::fabs(h[2][2]) > 0.0) {
            const double s = 1.0 / h[2][2];
            for (int j = 0; j < 3; ++j)
                for (int l = 0; l < 3; ++l) h[j][l] = s * h[j][l];
        }
        std::memcpy(&Hs[9 * (size_t)k], h, 72);
    }
    double t[3] = {-1.0 * t12[0], -1.0 * t12[1], -1.0 * t12[2]};
    const double normt = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (std::fabs(normt - 1.0) > 1e-4) {
        const double s = 1. / normt;
        for (int j = 0; j < 3; ++j) t[j] = t[j] * s;
    }
    double R[9], E[9];
    std::memcpy(R, rotq[q], 72);
    {
        const double s = 1. / std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        const double u[3] = {t[0] * s, t[1] * s, t[2] * s};
        const M3 sk = {{0, -u[2], u[1]}, {u[2], 0, -u[0]}, {-u[1], u[0], 0}};
        M3 Em;
        mul33(sk, rotq[q], Em);
        std::memcpy(E, Em, 72);
    }
    if (!finite_all(R, 9) || !finite_all(t, 3) || !finite_all(E, 9) || !finite_all(norms.data(), 3 * P) || !finite_all(Hs.data(), 9 * P)) return fail(4);
    std::memcpy(R_out, R, 72);
    std::memcpy(t_out, t, 24);
    std::memcpy(E_out, E, 72);
    std::memcpy(norms_out, norms.data(), (size_t)24 * P);
    std::memcpy(Hs_out, Hs.data(), (size_t)72 * P);
    return 0;
}

// building blocks for the numpy comparisons
extern "C" int hao_jacobi33(const double *a, int variant, double *d, double *v) {
    M3 A, V;
    std::memcpy(A, a, 72);
    const int ok = jacobi33(A, d, V, variant);
    std::memcpy(v, V, 72);
    return ok;
}
extern "C" int hao_solve_by_inverse(const double *a, const double *b, int n, double *m) {
    if (n < 1 || n > 32) return 0;
    return solve_by_inverse(a, b, m, n);
}

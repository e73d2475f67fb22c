// bundle_adjust.cpp -- poselib::refineStereoBA (P/source/pose_estim.cpp:1083-1348) over mlpl_refine_stereo_ba and poselib::refineMultCamBA
// (:1384-1735) over mlpl_refine_multicam_ba: the branch for correspondences in camera coordinates (motion and structure, calibrated cameras,
// first frame fixed, pseudo-Huber cost).  The options the library does not build are refused with one line and `false`, every argument
// untouched; no other algorithm is substituted.
#include <cmath>
#include <cstdint>
#include <iostream>
#include <string>
#include <vector>

#include "facade_internal.h"
#include "matchinglib_poselib/pose_estim.h"

namespace poselib {

namespace {
bool refuse(const char *what) {
    std::cout << "refineStereoBA (MI355X hot-path library): " << what << " is not built." << std::endl;
    return false;
}
}  // namespace

bool refineStereoBA(cv::InputArray p1_, cv::InputArray p2_, cv::InputOutputArray R_, cv::InputOutputArray t_, cv::InputOutputArray Q_,
                    cv::InputOutputArray K1_, cv::InputOutputArray K2_, bool pointsInImgCoords, cv::InputArray mask_, const double angleThresh,
                    const double t_norm_tresh, const double huber_thresh, const bool optimFocalOnly, const bool optimMotionOnly,
                    const bool fixCamMat, cv::InputOutputArray dist1, cv::InputOutputArray dist2) {
    // :1101-1106
    if (p1_.empty() || p2_.empty() || Q_.empty()) return false;
    if (p1_.rows() != p2_.rows() || p1_.rows() != Q_.rows()) return false;
    if (pointsInImgCoords) return refuse("pointsInImgCoords (BART = 2: intrinsics and distortion in the parameter vector)");
    if (optimMotionOnly) return refuse("optimMotionOnly");
    if (optimFocalOnly) return refuse("optimFocalOnly");
    if (fixCamMat) return refuse("fixCamMat");
    if (!dist1.empty() || !dist2.empty()) return refuse("dist1 / dist2");
    const cv::Mat p1 = p1_.getMat(), p2 = p2_.getMat(), K1 = K1_.getMat(), K2 = K2_.getMat();
    cv::Mat R = R_.getMat(), t = t_.getMat(), Q = Q_.getMat();
    CV_Assert(p1.type() == CV_64F && p2.type() == CV_64F && Q.type() == CV_64F && R.type() == CV_64F && t.type() == CV_64F);
    CV_Assert(p1.cols == 2 && p2.cols == 2 && Q.cols == 3 && R.rows == 3 && R.cols == 3 && t.rows * t.cols == 3);
    CV_Assert(K1.type() == CV_64F && K2.type() == CV_64F && K1.rows == 3 && K1.cols == 3 && K2.rows == 3 && K2.cols == 3);
    const int n = p1.rows;
    double th = huber_thresh;
    if (th < 0) th = 0.005;  // ROBUST_THRESH
    // :1195 -- (1,1) and (2,2): fy and the 1.0, not fx and fy; the reference's indices
    th = 4.0 * th / (std::sqrt((double)2) * (K1.at<double>(1, 1) + K1.at<double>(2, 2) + K2.at<double>(1, 1) + K2.at<double>(2, 2)));
    std::vector<double> a((size_t)n * 2), b((size_t)n * 2), q((size_t)n * 3);
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < 2; ++c) a[(size_t)i * 2 + c] = p1.at<double>(i, c), b[(size_t)i * 2 + c] = p2.at<double>(i, c);
        for (int c = 0; c < 3; ++c) q[(size_t)i * 3 + c] = Q.at<double>(i, c);
    }
    std::vector<uint8_t> m;
    if (!mask_.empty()) {
        const cv::Mat mask = mask_.getMat();
        CV_Assert(mask.type() == CV_8U && mask.rows * mask.cols == n);
        m.resize((size_t)n);
        for (int i = 0; i < n; ++i) m[i] = mask.rows == 1 ? mask.at<uint8_t>(0, i) : mask.at<uint8_t>(i, 0);
    }
    double Rv[9], tv[3];
    for (int i = 0; i < 9; ++i) Rv[i] = R.at<double>(i / 3, i % 3);
    for (int i = 0; i < 3; ++i) tv[i] = t.rows == 1 ? t.at<double>(0, i) : t.at<double>(i, 0);
    const int rc = mlpl_refine_stereo_ba(mlpl_facade_default_ctx(), a.data(), b.data(), n, m.empty() ? nullptr : m.data(), Rv, tv, q.data(), th,
                                         angleThresh, t_norm_tresh, nullptr);
    if (rc < 0) throw cv::Exception(std::string("mlpl_refine_stereo_ba: ") + mlpl_last_error());
    if (rc == 0) return false;  // failed or refused by the difference rule (:1199-1203, :1305-1312): t restored, R and Q as they were
    for (int i = 0; i < 9; ++i) R.at<double>(i / 3, i % 3) = Rv[i];
    for (int i = 0; i < 3; ++i) (t.rows == 1 ? t.at<double>(0, i) : t.at<double>(i, 0)) = tv[i];
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) Q.at<double>(i, c) = q[(size_t)i * 3 + c];
    return true;
}

namespace {
bool refuse_multicam(const char *what) {
    std::cout << "refineMultCamBA (MI355X hot-path library): " << what << " is not built." << std::endl;
    return false;
}
int area(const cv::Mat &m) { return m.rows * m.cols; }
}  // namespace

bool refineMultCamBA(cv::InputArray ps, cv::InputArray map3D, cv::InputOutputArray Rs, cv::InputOutputArray ts, cv::InputOutputArray Qs,
                     cv::InputOutputArray Ks, bool pointsInImgCoords, cv::InputArray masks, const double angleThresh, const double t_norm_tresh,
                     const double huber_thresh, const bool /*optimFocalOnly*/, const bool optimMotionOnly, const bool /*fixCamMat*/,
                     cv::InputOutputArray dists) {
    using std::cerr;
    using std::endl;
    // :1400-1420
    if (ps.empty() || Qs.empty() || map3D.empty() || Rs.empty() || ts.empty() || Ks.empty()) {
        cerr << "Some input variables to BA are empty. Skipping!" << endl;
        return false;
    }
    if (!ps.isMatVector() || !map3D.isMatVector() || !Rs.isMatVector() || !ts.isMatVector() || !Ks.isMatVector()) {
        cerr << "Inputs must be of type vector<Mat>. Skipping!" << endl;
        return false;
    }
    if (!Qs.isMat()) {
        cerr << "Input Qs must be of type Mat. Skipping!" << endl;
        return false;
    }
    cv::Mat Q = Qs.getMat();
    const int nr_Qs = Q.rows;
    if (nr_Qs < 15) {
        cerr << "Too less 3D points. Skipping!" << endl;
        return false;
    }
    // :1422-1488
    std::vector<cv::Mat> p2D_vec, map3D_vec, R_mvec, t_mvec, K_vec;
    ps.getMatVector(p2D_vec);
    map3D.getMatVector(map3D_vec);
    Rs.getMatVector(R_mvec);
    ts.getMatVector(t_mvec);
    Ks.getMatVector(K_vec);
    const size_t vecSi = p2D_vec.size();
    if (map3D_vec.size() != vecSi || R_mvec.size() != vecSi || t_mvec.size() != vecSi || K_vec.size() != vecSi) {
        cerr << "Inputs of type vector<Mat> must be of same size. Skipping!" << endl;
        return false;
    }
    bool haveMasks = false;
    std::vector<cv::Mat> kpMask_vec;
    if (!masks.empty()) {
        masks.getMatVector(kpMask_vec);
        if (kpMask_vec.size() != vecSi) {
            cerr << "Input masks of type vector<Mat> must be of same size as other inputs. Skipping!" << endl;
            return false;
        }
        for (size_t i = 0; i < kpMask_vec.size(); ++i)
            if (p2D_vec[i].rows != area(kpMask_vec[i])) {
                cerr << "Input mask " << i << " does not have the same size as corresponding 2D features. Skipping BA!" << endl;
                return false;
            }
        haveMasks = true;
    }
    for (size_t i = 0; i < map3D_vec.size(); ++i) {
        const cv::Mat &mp = map3D_vec[i];
        const int mapSi = area(mp);
        int ones = 0;  // cv::countNonZero: a byte is non-zero whatever its signedness
        for (int r = 0; r < mp.rows; ++r)
            for (int c = 0; c < mp.cols; ++c) ones += *(mp.data + (size_t)r * mp.step + (size_t)c * mp.elemSize()) != 0;
        const int pSi = haveMasks ? area(kpMask_vec[i]) : p2D_vec[i].rows;
        if (nr_Qs != mapSi) {
            cerr << "3D map " << i << " does not have the same size as number of available 3D points. Skipping BA!" << endl;
            return false;
        }
        if (ones != pSi) {
            cerr << "3D map " << i << " does not contain the same number of non-zero values as provided 2D correspondences. Skipping BA!" << endl;
            return false;
        }
        if (mp.type() != CV_8SC1) {
            cerr << "3D map " << i << " must be of type char. Skipping BA!" << endl;
            return false;
        }
    }
    if (!dists.empty()) {
        std::vector<cv::Mat> dist_mvec;
        dists.getMatVector(dist_mvec);
        if (dist_mvec.size() != vecSi) {
            cerr << "Input dists of type vector<Mat> must be of same size as other inputs. Skipping!" << endl;
            return false;
        }
    }
    // what the library does not build
    if (pointsInImgCoords) return refuse_multicam("pointsInImgCoords (intrinsics and distortion in the parameter vector)");
    if (optimMotionOnly) return refuse_multicam("optimMotionOnly");
    if (haveMasks)
        for (const cv::Mat &mk : kpMask_vec)
            for (int r = 0; r < mk.rows; ++r)
                for (int c = 0; c < mk.cols; ++c)
                    if (!mk.at<unsigned char>(r, c))
                        return refuse_multicam("masks with a zero entry (the reference reads past its compacted point list there)");
    const int m = (int)vecSi, n = nr_Qs;
    CV_Assert(Q.type() == CV_64F && Q.cols == 3);
    // :1510-1514, :1566-1571 -- (1,1) and (2,2): fy and the 1.0, the reference's indices
    double th = huber_thresh;
    if (th < 0) th = 0.005;  // ROBUST_THRESH
    double f_mean = 0;
    for (const cv::Mat &Kx : K_vec) {
        CV_Assert(Kx.type() == CV_64F && Kx.rows == 3 && Kx.cols == 3);
        f_mean += (Kx.at<double>(1, 1) + Kx.at<double>(2, 2)) / 2.0;
    }
    f_mean /= static_cast<double>(vecSi);
    th /= f_mean;
    // the dense layout of the C entry: ps[j] walks the non-zero entries of map3D[j] in ascending point order (BA_driver.cpp:2136-2157)
    std::vector<double> p((size_t)m * n * 2, 0.0), Rv((size_t)m * 9), tv((size_t)m * 3), q((size_t)n * 3);
    std::vector<uint8_t> vis((size_t)m * n, 0);
    for (int j = 0; j < m; ++j) {
        const cv::Mat &pj = p2D_vec[j], &mp = map3D_vec[j], &R = R_mvec[j], &t = t_mvec[j];
        CV_Assert(pj.type() == CV_64F && pj.cols == 2 && R.type() == CV_64F && R.rows == 3 && R.cols == 3 && t.type() == CV_64F && area(t) == 3);
        int at = 0;
        for (int i = 0; i < n; ++i) {
            const signed char seen = mp.rows == 1 ? mp.at<signed char>(0, i) : mp.at<signed char>(i / mp.cols, i % mp.cols);
            if (!seen) continue;
            vis[(size_t)j * n + i] = 1;
            p[((size_t)j * n + i) * 2] = pj.at<double>(at, 0), p[((size_t)j * n + i) * 2 + 1] = pj.at<double>(at, 1);
            ++at;
        }
        for (int i = 0; i < 9; ++i) Rv[(size_t)j * 9 + i] = R.at<double>(i / 3, i % 3);
        for (int i = 0; i < 3; ++i) tv[(size_t)j * 3 + i] = t.rows == 1 ? t.at<double>(0, i) : t.at<double>(i, 0);
    }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) q[(size_t)i * 3 + c] = Q.at<double>(i, c);
    const int rc = mlpl_refine_multicam_ba(mlpl_facade_default_ctx(), p.data(), vis.data(), m, n, Rv.data(), tv.data(), q.data(), th, angleThresh,
                                           t_norm_tresh, nullptr);
    if (rc < 0) throw cv::Exception(std::string("mlpl_refine_multicam_ba: ") + mlpl_last_error());
    if (rc == 0) return false;  // failed or refused by the difference rule (:1654-1716): every t restored, R and Q as they were
    for (int j = 0; j < m; ++j) {
        cv::Mat &R = R_mvec[j], &t = t_mvec[j];  // headers onto the caller's data
        for (int i = 0; i < 9; ++i) R.at<double>(i / 3, i % 3) = Rv[(size_t)j * 9 + i];
        for (int i = 0; i < 3; ++i) (t.rows == 1 ? t.at<double>(0, i) : t.at<double>(i, 0)) = tv[(size_t)j * 3 + i];
    }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) Q.at<double>(i, c) = q[(size_t)i * 3 + c];
    return true;
}

}  // namespace poselib

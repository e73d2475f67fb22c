// bundle_adjust.cpp -- poselib::refineStereoBA (P/source/pose_estim.cpp:1083-1348) over mlpl_refine_stereo_ba: the branch for correspondences
// in camera coordinates (motion and structure, calibrated cameras, first frame fixed, pseudo-Huber cost).  The options the library does not
// build are refused with one line and `false`, every argument untouched; no other algorithm is substituted.
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

}  // namespace poselib

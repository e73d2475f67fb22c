// gms.cpp -- filterMatchesGMS (M/source/gms.cpp) over mlpl_gms_filter.
#include "matchinglib_poselib/gms.h"

#include <cstdint>
#include <string>

#include "facade_internal.h"

namespace {

int run_gms(const std::vector<cv::KeyPoint> &keypoints1, const cv::Size &size1, const std::vector<cv::KeyPoint> &keypoints2, const cv::Size &size2,
            const std::vector<cv::DMatch> &matches, bool use_scale, bool use_rotation, std::vector<uint8_t> &keep) {
    static_assert(sizeof(cv::DMatch) == sizeof(mlpl_dmatch), "DMatch layout");
    std::vector<float> k1(2 * keypoints1.size()), k2(2 * keypoints2.size());
    for (size_t i = 0; i < keypoints1.size(); ++i) k1[2 * i] = keypoints1[i].pt.x, k1[2 * i + 1] = keypoints1[i].pt.y;
    for (size_t i = 0; i < keypoints2.size(); ++i) k2[2 * i] = keypoints2[i].pt.x, k2[2 * i + 1] = keypoints2[i].pt.y;
    if (matches.size() > 65535) throw cv::Exception("filterMatchesGMS: more than 65535 matches");
    keep.assign(matches.size(), 0);
    int n_keep = 0;
    const int rc = mlpl_gms_filter(mlpl_facade_default_ctx(), k1.data(), (int)keypoints1.size(), size1.width, size1.height, k2.data(),
                                   (int)keypoints2.size(), size2.width, size2.height, reinterpret_cast<const mlpl_dmatch *>(matches.data()),
                                   (int)matches.size(), use_scale ? 1 : 0, use_rotation ? 1 : 0, keep.data(), &n_keep, nullptr);
    if (rc != 0) throw cv::Exception(std::string("filterMatchesGMS: ") + mlpl_last_error());
    return n_keep;
}

}  // namespace

int filterMatchesGMS(const std::vector<cv::KeyPoint> &keypoints1, const cv::Size imageSize1, const std::vector<cv::KeyPoint> &keypoints2,
                     const cv::Size imageSize2, const std::vector<cv::DMatch> &matches, std::vector<bool> &inlierMask, const bool useScale,
                     const bool useRotation) {
    std::vector<uint8_t> keep;
    const int n = run_gms(keypoints1, imageSize1, keypoints2, imageSize2, matches, useScale, useRotation, keep);
    if (n > 0) inlierMask.assign(keep.begin(), keep.end());   // the reference assigns the mask only when a run beats the count 0
    return n;
}

int filterMatchesGMS(const std::vector<cv::KeyPoint> &keypoints1, const cv::Size imageSize1, const std::vector<cv::KeyPoint> &keypoints2,
                     const cv::Size imageSize2, const std::vector<cv::DMatch> &matches, std::vector<cv::DMatch> &matches_filtered,
                     const bool useScale, const bool useRotation) {
    std::vector<uint8_t> keep;
    const int n = run_gms(keypoints1, imageSize1, keypoints2, imageSize2, matches, useScale, useRotation, keep);
    matches_filtered.clear();
    matches_filtered.reserve((size_t)n);
    for (size_t i = 0; i < matches.size(); ++i)
        if (keep[i]) matches_filtered.push_back(matches[i]);
    return n;
}

// subpix.cpp -- matchinglib::getSubPixMatches (M/source/matchers.cpp:1085-1297) over mlpl_subpix_matches and
// matchinglib::getSubPixMatches_seperate_Imgs (matchers.cpp:1318-1391) over mlpl_subpix_separate.
#include <cstdint>
#include <iostream>
#include <string>

#include "facade_internal.h"
#include "matchinglib_poselib/matchinglib_matchers.h"

namespace matchinglib {

int getSubPixMatches(cv::Mat &img1, cv::Mat &img2, std::vector<cv::KeyPoint> *keypoints1, std::vector<cv::KeyPoint> *keypoints2,
                     std::vector<bool> *inliers) {
    if (keypoints1->size() != keypoints2->size()) {
        std::cout << "For subpixel-refinement the number of left and right keypoints must be the same as they must match!" << std::endl;
        return -2;
    }
    if (img1.empty() || img2.empty() || img1.type() != CV_8U || img2.type() != CV_8U)
        throw cv::Exception("getSubPixMatches: the images must be 8-bit, single channel and not empty");
    const size_t n = keypoints1->size();
    if (n > 65535) throw cv::Exception("getSubPixMatches: more than 65535 matches");
    std::vector<float> k1(2 * n), k2(2 * n), s1(n), s2(n);
    for (size_t i = 0; i < n; ++i) {
        const cv::KeyPoint &a = (*keypoints1)[i], &b = (*keypoints2)[i];
        k1[2 * i] = a.pt.x, k1[2 * i + 1] = a.pt.y, s1[i] = a.size;
        k2[2 * i] = b.pt.x, k2[2 * i + 1] = b.pt.y, s2[i] = b.size;
    }
    std::vector<uint8_t> mask(n, 0);
    int n_refined = 0, status = -1;
    const int rc = mlpl_subpix_matches(mlpl_facade_default_ctx(), img1.data, img1.cols, img1.rows, (size_t)img1.step, img2.data, img2.cols,
                                       img2.rows, (size_t)img2.step, k1.data(), k2.data(), s1.data(), s2.data(), (int)n, mask.data(),
                                       &n_refined, &status, nullptr);
    if (rc != 0) throw cv::Exception(std::string("getSubPixMatches: ") + mlpl_last_error());
    for (size_t i = 0; i < n; ++i) (*keypoints2)[i].pt = cv::Point2f(k2[2 * i], k2[2 * i + 1]);   // unchanged bits where nothing was refined
    if (inliers != NULL) inliers->assign(mask.begin(), mask.end());
    return status;
}

int getSubPixMatches_seperate_Imgs(cv::Mat &img1, cv::Mat &img2, std::vector<cv::KeyPoint> *keypoints1, std::vector<cv::KeyPoint> *keypoints2,
                                   std::vector<bool> *inliers) {
    if (keypoints1->size() != keypoints2->size()) {
        std::cout << "For subpixel-refinement the number of left and right keypoints must be the same as they must match!" << std::endl;
        return -2;
    }
    if (img1.empty() || img2.empty() || img1.type() != CV_8U || img2.type() != CV_8U)
        throw cv::Exception("getSubPixMatches_seperate_Imgs: the images must be 8-bit, single channel and not empty");
    const size_t n = keypoints1->size();
    if (n > 65535) throw cv::Exception("getSubPixMatches_seperate_Imgs: more than 65535 matches");
    std::vector<float> k1(2 * n), k2(2 * n), s1(n), s2(n);
    for (size_t i = 0; i < n; ++i) {
        const cv::KeyPoint &a = (*keypoints1)[i], &b = (*keypoints2)[i];
        k1[2 * i] = a.pt.x, k1[2 * i + 1] = a.pt.y, s1[i] = a.size;
        k2[2 * i] = b.pt.x, k2[2 * i + 1] = b.pt.y, s2[i] = b.size;
    }
    std::vector<uint8_t> mask(n, 0);
    int n_refined = 0, status = -1;
    const int rc = mlpl_subpix_separate(mlpl_facade_default_ctx(), img1.data, img1.cols, img1.rows, (size_t)img1.step, img2.data, img2.cols,
                                        img2.rows, (size_t)img2.step, k1.data(), k2.data(), s1.data(), s2.data(), (int)n, mask.data(), nullptr,
                                        &n_refined, &status, nullptr);
    if (rc != 0) throw cv::Exception(std::string("getSubPixMatches_seperate_Imgs: ") + mlpl_last_error());
    for (size_t i = 0; i < n; ++i) {   // unchanged bits where the match is no inlier
        (*keypoints1)[i].pt = cv::Point2f(k1[2 * i], k1[2 * i + 1]);
        (*keypoints2)[i].pt = cv::Point2f(k2[2 * i], k2[2 * i + 1]);
    }
    if (inliers != NULL) inliers->assign(mask.begin(), mask.end());
    return status;
}

}  // namespace matchinglib

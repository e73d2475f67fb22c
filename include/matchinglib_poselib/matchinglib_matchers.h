// matchinglib_matchers.h -- drop-in for the reference's matchinglib/include/matchinglib/matchinglib_matchers.h:61-64.
// Same name, arguments, defaults and return codes; the LINEAR (brute-force) matcher runs on the MI355X through
// libmlpl_hip.so (include/mlpl_c.h).  Every other matcher name returns -2 ("Matcher not supported"): those matchers are
// outside the hot path this library accelerates.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "matchinglib_poselib/cv_compat.h"

namespace matchinglib {

// Return value: 0 ok, -1 wrong input data, -2 matcher not supported, -3 matching failed (< 2 matches left),
// -4 too few keypoints (< 15).  Throws cv::Exception when descriptors1.type() != descriptors2.type() (CV_Assert,
// reference matchers.cpp:119).
int getMatches(const std::vector<cv::KeyPoint> &keypoints1, const std::vector<cv::KeyPoint> &keypoints2,
               cv::Mat const &descriptors1, cv::Mat const &descriptors2, cv::Size imgSi,
               std::vector<cv::DMatch> &finalMatches, std::string const &matcher_name = "GMBSOF", bool VFCrefine = false,
               bool ratioTest = true, std::string const &descriptor_name = "", std::string idxPars_NMSLIB = "",
               std::string queryPars_NMSLIB = "", const size_t nr_threads = 0);

// Sub-pixel refinement of matched keypoints by template matching (reference matchinglib_matchers.h:86, matchers.cpp:1085-1297), through
// mlpl_subpix_matches (include/mlpl_c.h states what is computed and the declared deviations: an exact-integer difference table, and matches
// the reference would assert on are dropped).  keypoints1[i] matches keypoints2[i]; the refined positions are written to keypoints2, the
// inlier mask to *inliers when given.  Return value: 0 ok, -1 refinement failed for too many keypoints (fewer than a third, or fewer than 2,
// were refined; keypoints2 and *inliers are written all the same), -2 the keypoint sets differ in size.  Throws cv::Exception for images
// that are not 8-bit single channel (the reference's matchTemplate accepts float images too) and for more than 65535 keypoints.
int getSubPixMatches(cv::Mat &img1, cv::Mat &img2, std::vector<cv::KeyPoint> *keypoints1, std::vector<cv::KeyPoint> *keypoints2,
                     std::vector<bool> *inliers = NULL);

// Sub-pixel refinement of matched keypoints by cv::cornerSubPix on each image on its own (reference matchinglib_matchers.h:90,
// matchers.cpp:1318-1391; subPixRefine == 2, the variant for large rotations and scale changes), through mlpl_subpix_separate
// (include/mlpl_c.h restates cv::cornerSubPix and declares the deviations).  keypoints1[i] matches keypoints2[i]; a match whose two points
// both stay within sqrt(12) px takes its refined positions in BOTH lists and is an inlier.  Return value: 0 ok, -1 fewer than a third, or
// fewer than 2, of the matches are inliers (keypoints and *inliers are written all the same), -2 the keypoint sets differ in size.  Throws
// cv::Exception for images that are not 8-bit single channel, for an image smaller than 2 w + 5 pixels and for more than 65535 keypoints.
int getSubPixMatches_seperate_Imgs(cv::Mat &img1, cv::Mat &img2, std::vector<cv::KeyPoint> *keypoints1, std::vector<cv::KeyPoint> *keypoints2,
                                   std::vector<bool> *inliers = NULL);

}  // namespace matchinglib

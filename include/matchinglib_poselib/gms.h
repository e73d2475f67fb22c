// gms.h -- drop-in for the reference's matchinglib/include/matchinglib/gms.h: the GMS (grid-based motion statistics) match filter, the step
// getCorrespondences runs behind getMatches.  Same names, arguments and return value (the number of inliers); the work runs on the MI355X
// through mlpl_gms_filter (include/mlpl_c.h, which lists the reference's quirks that are reproduced and the out-of-bounds cases that are not).
// Like the reference's, the functions live in the global namespace.
#pragma once
#include <vector>

#include "matchinglib_poselib/cv_compat.h"

// inlierMask is assigned only when at least one inlier was found: on a return of 0 it is left untouched (MatchGMS::getInlierMask).
int filterMatchesGMS(const std::vector<cv::KeyPoint> &keypoints1, const cv::Size imageSize1, const std::vector<cv::KeyPoint> &keypoints2,
                     const cv::Size imageSize2, const std::vector<cv::DMatch> &matches, std::vector<bool> &inlierMask,
                     const bool useScale = false, const bool useRotation = false);

// matches_filtered receives the inliers in order; it is empty on a return of 0.
int filterMatchesGMS(const std::vector<cv::KeyPoint> &keypoints1, const cv::Size imageSize1, const std::vector<cv::KeyPoint> &keypoints2,
                     const cv::Size imageSize2, const std::vector<cv::DMatch> &matches, std::vector<cv::DMatch> &matches_filtered,
                     const bool useScale = false, const bool useRotation = false);

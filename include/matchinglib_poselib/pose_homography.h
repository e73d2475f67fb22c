// pose_homography.h -- the two self-contained functions of the reference's poselib/pose_homography.h on the MI355X:
// computeHomographyArrsac and estimateMultHomographys (P/source/pose_homography.cpp:291-555), with the reference's signatures and
// defaults.  estimatePoseHomographies (the Halign option) is not provided.
//
// Shapes: without OpenCV (cv_compat.h: single-channel matrices only) the points are n x 2 CV_64F, the single-channel view of the
// reference's n x 1 CV_64FC2; estimateMultHomographys takes n x 2 CV_64F as in the reference.  A wrong shape throws cv::Exception
// (the reference's CV_Assert).  Both functions draw from the process-wide pair of cv::RNG streams that estimateEssentialMat's ARRSAC uses
// (setArrsacRngState / getArrsacRngState, pose_estim.h): in the reference the samplers' streams are function-local statics shared by
// every theia::Arrsac instantiation.
#pragma once
#include <utility>
#include <vector>

#include "matchinglib_poselib/cv_compat.h"

namespace poselib {

// th: inlier threshold; H: 3 x 3 CV_64F (refined on the inliers); mask: 1 x n CV_8U (from before the refinement); p_filtered1 / 2: the
// inliers, rows x 2 CV_64F -- written only when both are requested.  Returns false when no homography was found (outputs untouched).
bool computeHomographyArrsac(cv::InputArray points1, cv::InputArray points2, cv::OutputArray H, double th, cv::OutputArray mask = cv::noArray(),
                             cv::OutputArray p_filtered1 = cv::noArray(), cv::OutputArray p_filtered2 = cv::noArray());

// Every output is optional (nullptr).  Returns 0, or -1 when the first plane was not found.  When more than one plane was found the
// results are APPENDED to the caller's vectors in descending order of the inlier count; otherwise the vectors are assigned (the reference's
// behaviour, :413-460).  As in the reference the ordering needs num_inl: without it the planes stay in the order they were found.
int estimateMultHomographys(cv::InputArray p1, cv::InputArray p2, double th, std::vector<cv::Mat> *inl_mask = nullptr,
                            std::vector<std::pair<cv::Mat, cv::Mat>> *inl_points = nullptr, std::vector<cv::Mat> *Hs = nullptr,
                            std::vector<unsigned int> *num_inl = nullptr, bool varTh = true, std::vector<double> *planeStrength = nullptr,
                            unsigned int maxPlanes = 0, unsigned int minPtsPerPlane = 4);

}  // namespace poselib

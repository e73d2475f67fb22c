// pose_homography.h -- the reference's poselib/pose_homography.h on the MI355X: estimatePoseHomographies (the pose of a scene of
// planes by homography alignment, what the harnesses' --Halign calls), computeHomographyArrsac and estimateMultHomographys
// (P/source/pose_homography.cpp:127-555), with the reference's signatures and defaults.  StereoRefine's Halign switch is not wired to
// it yet (it keeps returning -1 with its message).
//
// Shapes: without OpenCV (cv_compat.h: single-channel matrices only) the points are n x 2 CV_64F, the single-channel view of the
// reference's n x 1 CV_64FC2; estimateMultHomographys takes n x 2 CV_64F as in the reference.  A wrong shape throws cv::Exception
// (the reference's CV_Assert).  All three functions draw from the process-wide pair of cv::RNG streams that estimateEssentialMat's ARRSAC uses
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

// Return value as in the reference: 0; -1 no plane found; -2 the planes are too weak (checkPlaneStrength: the strengths above 0.1 must sum
// to more than 0.5); -3 the homography alignment failed (one plane only, a pure rotation, ...: mlpl_c.h lists the cases); -4 R or t was
// not requested (checked after the alignment, as in the reference).  p1, p2: n x 2 CV_64F in camera coordinates.  R (3 x 3), t (3 x 1),
// E (3 x 3, optional) CV_64F; inliers and mask (1 x n CV_8U): computeReprojError2 < th^2 over all n rows.  A non-empty mask on entry
// selects the rows the planes are searched in.  The optional vectors are assigned (not appended to) on success only.
int estimatePoseHomographies(cv::InputArray p1, cv::InputArray p2, cv::OutputArray R, cv::OutputArray t, cv::OutputArray E, double th, int &inliers,
                             cv::InputOutputArray mask = cv::noArray(), bool checkPlaneStrength = false, bool varTh = false,
                             std::vector<std::pair<cv::Mat, cv::Mat>> *inlier_points = nullptr, std::vector<unsigned int> *numbersHinliers = nullptr,
                             std::vector<cv::Mat> *homographies = nullptr, std::vector<double> *planeStrengths = nullptr);

}  // namespace poselib

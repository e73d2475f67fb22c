// pose_linear_refinement.h -- drop-in for the reference's poselib/include/poselib/pose_linear_refinement.h: refineEssentialLinear with the same
// name, argument order, defaults and return value.  The refit runs on the MI355X through libmlpl_hip.so (mlpl_refine_essential_linear and,
// for PR_KNEIP, mlpl_refine_essential_linear_rt; include/mlpl_c.h lists the deviations).
#pragma once
#include <cstddef>

#include "matchinglib_poselib/cv_compat.h"
#include "matchinglib_poselib/pose_estim.h"

namespace poselib {

// Iteratively re-weighted linear refinement of E on the inliers in `mask` (pose_linear_refinement.cpp:85-309).  refineMethod = a solver of
// RefinePostAlg (PR_8PT, PR_NISTER, PR_STEWENIUS, PR_KNEIP) OR-ed with a weighting (PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS, PR_NO_WEIGHTS).  p1, p2: n x 2
// CV_64F camera coordinates; E: 3 x 3 CV_64F (in / out); mask: 1 x n CV_8U (in / out).  Returns false (E and mask untouched) with fewer
// than 6 inliers or when the first step loses more than maxRelativeInlierCntLoss of them.  With PR_8PT / PR_NISTER / PR_STEWENIUS a passed R
// is cleared (they yield no rotation); t is cleared only when R is not requested.
// PR_KNEIP (OpenGV's eigensolver on the inliers; the weighting changes nothing, as in the reference) runs when BOTH R and t are requested:
// R (3 x 3 CV_64F) is the start rotation -- empty or no rotation: up to 12 starts near the identity, drawn from the seed setRansacSeed
// fixes (the reference draws from the process-wide rand()) -- and R, t (3 x 1, unit length) receive the pose of the last accepted step;
// when no step was accepted the call still returns true with E unchanged and R cleared, as the reference does.  Deviation: without R or
// without t PR_KNEIP returns false with a message and everything untouched (the reference refines E and drops the pose).
bool refineEssentialLinear(cv::InputArray p1, cv::InputArray p2, cv::InputOutputArray E, cv::InputOutputArray mask,
                           int refineMethod,  // a combination of poselib::RefinePostAlg
                           size_t &nr_inliers, cv::InputOutputArray R = cv::noArray(), cv::OutputArray t = cv::noArray(), double th = 0.008,
                           size_t num_iterative_steps = 4, double threshold_multiplier = 2.0, double pseudoHuberThreshold_multiplier = 0.1,
                           double maxRelativeInlierCntLoss = 0.15);

}  // namespace poselib

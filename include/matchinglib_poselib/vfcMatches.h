// vfcMatches.h -- drop-in for the reference's matchinglib/include/matchinglib/vfcMatches.h: the vector field consensus (VFC) match filter,
// the step getMatches runs when VFCrefine is true.  Same name, arguments and return codes; the work runs on the MI355X through
// mlpl_vfc_filter (include/mlpl_c.h, which states what "equal to the reference" means for this filter).
#pragma once
#include <vector>

#include "matchinglib_poselib/cv_compat.h"

namespace matchinglib {

// Return value: 0 ok, -1 too few matches (< 5: prints "Too less matches for refinement with VFC!", matches_out empty), -2 fewer than
// 10 % of the matches were kept ("maybe VFC failed"; matches_out holds them).
int filterWithVFC(std::vector<cv::KeyPoint> const &keypL, std::vector<cv::KeyPoint> const &keypR, std::vector<cv::DMatch> const &matches_in,
                  std::vector<cv::DMatch> &matches_out);

// The reference draws VFC's control points with rand() from wherever the process-wide stream stands.  Here the filter draws from the
// start of srand(seed): seed 1 by default (glibc's state when srand was never called); setVfcSeed(s) chooses another, clearVfcSeed()
// returns to 1.  Thread-local, used by filterWithVFC and getMatches(VFCrefine = true).
void setVfcSeed(unsigned seed);
void clearVfcSeed();

}  // namespace matchinglib

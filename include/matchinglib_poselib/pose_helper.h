// pose_helper.h -- the stereo rectification exports of the reference's poselib/pose_helper.h on the MI355X: getRectificationParameters and
// GetRectifiedImages with the reference's signatures and defaults (P/source/pose_helper.cpp:1366-1422, :2775-2793), and two documented
// extensions that keep a harness on the device without OpenCV's imgproc: initUndistortRectifyMap (OpenCV's argument list, so a harness
// changes only the namespace) and rectifyImages (the fused call on a pair).  The arithmetic, what is pinned and the declared deviations:
// include/mlpl_c.h, "stereo rectification".  Not built: the stereoRectify2 branch, estimateOptimalFocalScale, estimateVergence,
// ShowRectifiedImages.
//
// Shapes: matrices are CV_64F (R, K1, K2, Rect, Knew 3 x 3; t 3 x 1 or 1 x 3; distortion coefficients 4, 5 or 8 values in a row or a
// column, or empty = none; P 3 x 4); images CV_8U single channel; maps CV_32F.  A wrong matrix shape or type throws cv::Exception (the
// reference's CV_Assert / at<double>).
#pragma once
#include "matchinglib_poselib/cv_compat.h"

namespace poselib {

// Returns 0.  globRectFunct = true: the method of Fusiello, Trucco and Verri.  globRectFunct = false (the stereoRectify2 branch) is not
// built: the function prints that, returns -1 and writes no output; it never substitutes the Fusiello result.  K2new receives a copy of
// K1new; roi1 the valid rectangle; roi2 is left as it is (the reference assigns its local pointer only).
int getRectificationParameters(cv::InputArray R, cv::InputArray t, cv::InputArray K1, cv::InputArray K2, cv::InputArray distcoeffs1,
                               cv::InputArray distcoeffs2, const cv::Size &imageSize, cv::OutputArray Rect1, cv::OutputArray Rect2,
                               cv::OutputArray K1new, cv::OutputArray K2new, double alpha = -1, bool globRectFunct = true,
                               const cv::Size &newImgSize = cv::Size(), cv::Rect *roi1 = nullptr, cv::Rect *roi2 = nullptr,
                               cv::OutputArray P1new = cv::noArray(), cv::OutputArray P2new = cv::noArray());

// remap(img, out, mapX, mapY, INTER_LINEAR, BORDER_CONSTANT) on both images.  Returns 0; -1 (with a message, outputs untouched) when an
// image is not 8-bit single channel or a map is not CV_32F.  The outputs take the size of their maps; t and newImgSize are unused, as in
// the reference.
int GetRectifiedImages(cv::InputArray img1, cv::InputArray img2, cv::InputArray mapX1, cv::InputArray mapY1, cv::InputArray mapX2,
                       cv::InputArray mapY2, cv::InputArray t, cv::OutputArray outImg1, cv::OutputArray outImg2, cv::Size newImgSize = cv::Size());

// Extension: cv::initUndistortRectifyMap.  m1type must be CV_32FC1 (anything else throws cv::Exception); an empty R is the identity, an
// empty newCameraMatrix is cameraMatrix.
void initUndistortRectifyMap(cv::InputArray cameraMatrix, cv::InputArray distCoeffs, cv::InputArray R, cv::InputArray newCameraMatrix, cv::Size size,
                             int m1type, cv::OutputArray map1, cv::OutputArray map2);

// Extension: both rectified images in one fused launch, no map in memory; byte for byte what initUndistortRectifyMap followed by
// GetRectifiedImages gives.  newImgSize = (0, 0): the image size.  Returns 0; -1 when an image is not 8-bit single channel or the two
// sizes differ.
int rectifyImages(cv::InputArray img1, cv::InputArray img2, cv::InputArray K1, cv::InputArray distcoeffs1, cv::InputArray Rect1, cv::InputArray K2,
                  cv::InputArray distcoeffs2, cv::InputArray Rect2, cv::InputArray Knew, cv::OutputArray outImg1, cv::OutputArray outImg2,
                  cv::Size newImgSize = cv::Size());

}  // namespace poselib

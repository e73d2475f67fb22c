// pose_helper.cpp -- poselib::getRectificationParameters (P/source/pose_helper.cpp:1366-1422) over mlpl_rectify_parameters,
// poselib::GetRectifiedImages (:2775-2793) over mlpl_remap_bilinear, and the extensions poselib::initUndistortRectifyMap
// (mlpl_rectify_maps) and poselib::rectifyImages (mlpl_rectify_images).
#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "facade_internal.h"
#include "matchinglib_poselib/pose_helper.h"

namespace {

// the values of a CV_64F matrix in row-major order; `what` names it in the exception
std::vector<double> doubles_of(const cv::Mat &m, const char *what) {
    if (m.type() != CV_64F) throw cv::Exception(std::string(what) + " must be CV_64F");
    std::vector<double> v;
    v.reserve((size_t)m.rows * m.cols);
    for (int r = 0; r < m.rows; ++r)
        for (int c = 0; c < m.cols; ++c) v.push_back(m.at<double>(r, c));
    return v;
}

std::vector<double> matrix_of(cv::InputArray a, int rows, int cols, const char *what) {
    const cv::Mat m = a.getMat();
    if (m.empty() || !((m.rows == rows && m.cols == cols) || (cols == 1 && m.rows == 1 && m.cols == rows)))
        throw cv::Exception(std::string(what) + " has the wrong shape");
    return doubles_of(m, what);
}

std::vector<double> coefficients_of(cv::InputArray a, const char *what) {
    if (a.empty()) return {};
    const cv::Mat m = a.getMat();
    const size_t n = (size_t)m.rows * m.cols;
    if (!(m.rows == 1 || m.cols == 1) || !(n == 4 || n == 5 || n == 8)) throw cv::Exception(std::string(what) + " must hold 4, 5 or 8 coefficients");
    return doubles_of(m, what);
}

void put(cv::OutputArray out, int rows, int cols, const double *v) {
    out.create(rows, cols, CV_64F);
    cv::Mat m = out.getMat();
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m.at<double>(r, c) = v[r * cols + c];
}

bool is_u8(const cv::Mat &m) { return !m.empty() && m.type() == CV_8U; }

// {K[9], dist[8], Rect[9], Knew[9]}
void param_block(double *p, const std::vector<double> &K, const std::vector<double> &d, const std::vector<double> &Rect, const std::vector<double> &Knew) {
    std::memcpy(p, K.data(), 72);
    for (int i = 0; i < 8; ++i) p[9 + i] = i < (int)d.size() ? d[i] : 0.0;
    std::memcpy(p + 17, Rect.data(), 72);
    std::memcpy(p + 26, Knew.data(), 72);
}

}  // namespace

namespace poselib {

int getRectificationParameters(cv::InputArray R, cv::InputArray t, cv::InputArray K1, cv::InputArray K2, cv::InputArray distcoeffs1,
                               cv::InputArray distcoeffs2, const cv::Size &imageSize, cv::OutputArray Rect1, cv::OutputArray Rect2,
                               cv::OutputArray K1new, cv::OutputArray K2new, double alpha, bool globRectFunct, const cv::Size &newImgSize,
                               cv::Rect *roi1, cv::Rect * /*roi2: the reference assigns its local pointer only*/, cv::OutputArray P1new,
                               cv::OutputArray P2new) {
    CV_Assert(!R.empty() && !t.empty() && !K1.empty() && !K2.empty() && (!P1new.needed() || globRectFunct) && (!P2new.needed() || globRectFunct));
    if (!globRectFunct) {
        std::cout << "getRectificationParameters: the stereoRectify2 branch (globRectFunct = false) is not built" << std::endl;
        return -1;
    }
    const std::vector<double> r = matrix_of(R, 3, 3, "R"), tv = matrix_of(t, 3, 1, "t"), k1 = matrix_of(K1, 3, 3, "K1"), k2 = matrix_of(K2, 3, 3, "K2"),
                              d1 = coefficients_of(distcoeffs1, "distcoeffs1"), d2 = coefficients_of(distcoeffs2, "distcoeffs2");
    double rect1[9], rect2[9], knew[9], p1[12], p2[12];
    int roi[4];
    const int rc = mlpl_rectify_parameters(r.data(), tv.data(), k1.data(), k2.data(), d1.empty() ? nullptr : d1.data(), (int)d1.size(),
                                           d2.empty() ? nullptr : d2.data(), (int)d2.size(), imageSize.width, imageSize.height, alpha,
                                           newImgSize.width, newImgSize.height, rect1, rect2, knew, roi, p1, p2, nullptr);
    if (rc != 0) throw cv::Exception(std::string("getRectificationParameters: ") + mlpl_last_error());
    put(Rect1, 3, 3, rect1);
    put(Rect2, 3, 3, rect2);
    put(K1new, 3, 3, knew);
    put(K2new, 3, 3, knew);
    if (roi1) *roi1 = cv::Rect(roi[0], roi[1], roi[2], roi[3]);
    if (P1new.needed()) put(P1new, 3, 4, p1);
    if (P2new.needed()) put(P2new, 3, 4, p2);
    return 0;
}

void initUndistortRectifyMap(cv::InputArray cameraMatrix, cv::InputArray distCoeffs, cv::InputArray R, cv::InputArray newCameraMatrix, cv::Size size,
                             int m1type, cv::OutputArray map1, cv::OutputArray map2) {
    if (m1type != CV_32FC1) throw cv::Exception("initUndistortRectifyMap: only CV_32FC1 maps are built");
    const std::vector<double> K = matrix_of(cameraMatrix, 3, 3, "cameraMatrix"), d = coefficients_of(distCoeffs, "distCoeffs");
    const std::vector<double> Rm = R.empty() ? std::vector<double>{1, 0, 0, 0, 1, 0, 0, 0, 1} : matrix_of(R, 3, 3, "R");
    const std::vector<double> Kn = newCameraMatrix.empty() ? K : matrix_of(newCameraMatrix, 3, 3, "newCameraMatrix");
    if (size.width < 1 || size.height < 1) throw cv::Exception("initUndistortRectifyMap: the size must be positive");
    map1.create(size.height, size.width, CV_32F);
    map2.create(size.height, size.width, CV_32F);
    cv::Mat mx = map1.getMat(), my = map2.getMat();
    const int rc = mlpl_rectify_maps(mlpl_facade_default_ctx(), K.data(), d.empty() ? nullptr : d.data(), (int)d.size(), Rm.data(), Kn.data(), size.width,
                                     size.height, mx.ptr<float>(), my.ptr<float>());
    if (rc != 0) throw cv::Exception(std::string("initUndistortRectifyMap: ") + mlpl_last_error());
}

int GetRectifiedImages(cv::InputArray img1, cv::InputArray img2, cv::InputArray mapX1, cv::InputArray mapY1, cv::InputArray mapX2,
                       cv::InputArray mapY2, cv::InputArray t, cv::OutputArray outImg1, cv::OutputArray outImg2, cv::Size /*newImgSize*/) {
    CV_Assert(!img1.empty() && !img2.empty() && !mapX1.empty() && !mapY1.empty() && !mapX2.empty() && !mapY2.empty() && !t.empty());
    CV_Assert((img1.rows() == img2.rows()) && (img1.cols() == img2.cols()));
    const cv::Mat im[2] = {img1.getMat(), img2.getMat()};
    cv::Mat mx[2] = {mapX1.getMat(), mapX2.getMat()}, my[2] = {mapY1.getMat(), mapY2.getMat()};
    if (!is_u8(im[0]) || !is_u8(im[1])) {
        std::cout << "GetRectifiedImages: the images must be 8-bit, single channel" << std::endl;
        return -1;
    }
    for (int i = 0; i < 2; ++i) {
        if (mx[i].type() != CV_32F || my[i].type() != CV_32F) {
            std::cout << "GetRectifiedImages: the maps must be CV_32FC1" << std::endl;
            return -1;
        }
        CV_Assert(mx[i].rows == my[i].rows && mx[i].cols == my[i].cols);
        if (!mx[i].isContinuous()) mx[i] = mx[i].clone();
        if (!my[i].isContinuous()) my[i] = my[i].clone();
    }
    outImg1.create(mx[0].rows, mx[0].cols, CV_8U);
    outImg2.create(mx[1].rows, mx[1].cols, CV_8U);
    cv::Mat out[2] = {outImg1.getMat(), outImg2.getMat()};
    for (int i = 0; i < 2; ++i) {
        const int rc = mlpl_remap_bilinear(mlpl_facade_default_ctx(), im[i].data, im[i].cols, im[i].rows, (size_t)im[i].step, mx[i].ptr<float>(),
                                           my[i].ptr<float>(), mx[i].cols, mx[i].rows, out[i].data, (size_t)out[i].step);
        if (rc != 0) throw cv::Exception(std::string("GetRectifiedImages: ") + mlpl_last_error());
    }
    return 0;
}

int rectifyImages(cv::InputArray img1, cv::InputArray img2, cv::InputArray K1, cv::InputArray distcoeffs1, cv::InputArray Rect1, cv::InputArray K2,
                  cv::InputArray distcoeffs2, cv::InputArray Rect2, cv::InputArray Knew, cv::OutputArray outImg1, cv::OutputArray outImg2,
                  cv::Size newImgSize) {
    cv::Mat a = img1.getMat(), b = img2.getMat();
    if (!is_u8(a) || !is_u8(b) || a.rows != b.rows || a.cols != b.cols) {
        std::cout << "rectifyImages: the images must be 8-bit, single channel and of one size" << std::endl;
        return -1;
    }
    if (a.step != b.step) a = a.clone(), b = b.clone();
    const std::vector<double> kn = matrix_of(Knew, 3, 3, "Knew");
    double params[2 * 35];
    param_block(params, matrix_of(K1, 3, 3, "K1"), coefficients_of(distcoeffs1, "distcoeffs1"), matrix_of(Rect1, 3, 3, "Rect1"), kn);
    param_block(params + 35, matrix_of(K2, 3, 3, "K2"), coefficients_of(distcoeffs2, "distcoeffs2"), matrix_of(Rect2, 3, 3, "Rect2"), kn);
    const int ow = newImgSize.width * newImgSize.height != 0 ? newImgSize.width : a.cols, oh = newImgSize.width * newImgSize.height != 0 ? newImgSize.height : a.rows;
    outImg1.create(oh, ow, CV_8U);
    outImg2.create(oh, ow, CV_8U);
    cv::Mat o1 = outImg1.getMat(), o2 = outImg2.getMat();
    const int rc = mlpl_rectify_images(mlpl_facade_default_ctx(), a.data, b.data, a.cols, a.rows, (size_t)a.step, params, ow, oh, o1.data, o2.data,
                                       (size_t)o1.step);
    if (rc != 0) throw cv::Exception(std::string("rectifyImages: ") + mlpl_last_error());
    return 0;
}

}  // namespace poselib

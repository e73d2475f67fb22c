// rectify_facade.cpp -- poselib::getRectificationParameters, initUndistortRectifyMap, GetRectifiedImages and rectifyImages through the C++
// drop-in, called with the reference's signatures (tests/test_gpu_rectify_facade.py runs it and compares with the oracle and the C entries).
// argv[1]: input file {int32 width, height, step, new_width, new_height, n_dist1, n_dist2, 0; double alpha, R[9], t[3], K1[9], K2[9],
//          dist1[n_dist1], dist2[n_dist2]; uint8 img1[height][step], img2[height][step]}; the images are headers onto these rows.
// argv[2]: output file, in this order
//   int32 rc; double Rect1[9], Rect2[9], K1new[9], K2new[9], P1[12], P2[12]; int32 roi1[4], roi2[4]      the full call (roi2 handed in as 7, 7, 7, 7)
//   int32 rc; double Rect1[9], Rect2[9], K1new[9]                                                        the call with every default
//   int32 rc; int32 untouched                                                                            globRectFunct = false
//   int32 out_width, out_height; float mapx1, mapy1, mapx2, mapy2 [out_height][out_width]                initUndistortRectifyMap
//   int32 rc; uint8 out1, out2 [out_height][out_width]                                                   GetRectifiedImages
//   int32 rc; uint8 out1, out2 [out_height][out_width]                                                   rectifyImages
//   int32 rc of GetRectifiedImages on a CV_32F image, rc of rectifyImages on one, rc of GetRectifiedImages on CV_64F maps,
//         1 if initUndistortRectifyMap threw on CV_64F maps
#include <cstdint>
#include <cstdio>
#include <vector>

#include "matchinglib_poselib/pose_helper.h"

static cv::Mat mat64(int r, int c, const double *v) {
    cv::Mat m(r, c, CV_64F);
    for (int i = 0; i < r * c; ++i) m.at<double>(i / c, i % c) = v[i];
    return m;
}

static void put64(FILE *o, const cv::Mat &m) {
    for (int r = 0; r < m.rows; ++r) std::fwrite(m.ptr<double>(r), 8, m.cols, o);
}

template <typename T>
static void put_rows(FILE *o, const cv::Mat &m) {
    for (int r = 0; r < m.rows; ++r) std::fwrite(m.ptr<T>(r), sizeof(T), m.cols, o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    double alpha, v[30];
    if (std::fread(hd, 4, 8, f) != 8 || std::fread(&alpha, 8, 1, f) != 1 || std::fread(v, 8, 30, f) != 30) return 2;
    const int w = hd[0], h = hd[1], step = hd[2], nw = hd[3], nh = hd[4], n1 = hd[5], n2 = hd[6];
    std::vector<double> d1(n1), d2(n2);
    std::vector<uint8_t> b1((size_t)h * step), b2((size_t)h * step);
    if ((n1 && std::fread(d1.data(), 8, n1, f) != (size_t)n1) || (n2 && std::fread(d2.data(), 8, n2, f) != (size_t)n2) ||
        std::fread(b1.data(), 1, b1.size(), f) != b1.size() || std::fread(b2.data(), 1, b2.size(), f) != b2.size())
        return 2;
    std::fclose(f);
    const cv::Mat R = mat64(3, 3, v), t = mat64(3, 1, v + 9), K1 = mat64(3, 3, v + 12), K2 = mat64(3, 3, v + 21);
    const cv::Mat D1 = n1 ? mat64(n1, 1, d1.data()) : cv::Mat(), D2 = n2 ? mat64(1, n2, d2.data()) : cv::Mat();
    cv::Mat img1(h, w, CV_8U, b1.data(), (size_t)step), img2(h, w, CV_8U, b2.data(), (size_t)step);
    const cv::Size size(w, h), new_size(nw, nh);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;

    // ---- the full call
    cv::Mat Rect1, Rect2, K1new, K2new, P1, P2;
    cv::Rect roi1, roi2(7, 7, 7, 7);
    int32_t rc = poselib::getRectificationParameters(R, t, K1, K2, D1, D2, size, Rect1, Rect2, K1new, K2new, alpha, true, new_size, &roi1, &roi2, P1, P2);
    std::fwrite(&rc, 4, 1, o);
    put64(o, Rect1), put64(o, Rect2), put64(o, K1new), put64(o, K2new), put64(o, P1), put64(o, P2);
    const int32_t rois[8] = {roi1.x, roi1.y, roi1.width, roi1.height, roi2.x, roi2.y, roi2.width, roi2.height};
    std::fwrite(rois, 4, 8, o);

    // ---- every default: alpha = -1, globRectFunct = true, newImgSize = Size(), no roi, no P
    cv::Mat Ra, Rb, Ka, Kb;
    rc = poselib::getRectificationParameters(R, t, K1, K2, D1, D2, size, Ra, Rb, Ka, Kb);
    std::fwrite(&rc, 4, 1, o);
    put64(o, Ra), put64(o, Rb), put64(o, Ka);

    // ---- globRectFunct = false: -1, nothing written
    cv::Mat Rc, Rd, Kc, Kd;
    cv::Rect roi3(7, 7, 7, 7);
    rc = poselib::getRectificationParameters(R, t, K1, K2, D1, D2, size, Rc, Rd, Kc, Kd, alpha, false, new_size, &roi3);
    const int32_t untouched = Rc.empty() && Rd.empty() && Kc.empty() && Kd.empty() && roi3.x == 7 && roi3.width == 7;
    std::fwrite(&rc, 4, 1, o);
    std::fwrite(&untouched, 4, 1, o);

    // ---- maps, rectified images, the fused call
    const cv::Size out_size = nw * nh != 0 ? new_size : size;
    cv::Mat mx1, my1, mx2, my2, o1, o2, f1, f2;
    poselib::initUndistortRectifyMap(K1, D1, Rect1, K1new, out_size, CV_32FC1, mx1, my1);
    poselib::initUndistortRectifyMap(K2, D2, Rect2, K2new, out_size, CV_32FC1, mx2, my2);
    const int32_t os[2] = {out_size.width, out_size.height};
    std::fwrite(os, 4, 2, o);
    put_rows<float>(o, mx1), put_rows<float>(o, my1), put_rows<float>(o, mx2), put_rows<float>(o, my2);
    rc = poselib::GetRectifiedImages(img1, img2, mx1, my1, mx2, my2, t, o1, o2);
    std::fwrite(&rc, 4, 1, o);
    put_rows<uint8_t>(o, o1), put_rows<uint8_t>(o, o2);
    rc = poselib::rectifyImages(img1, img2, K1, D1, Rect1, K2, D2, Rect2, K1new, f1, f2, new_size);
    std::fwrite(&rc, 4, 1, o);
    put_rows<uint8_t>(o, f1), put_rows<uint8_t>(o, f2);

    // ---- refused types
    cv::Mat fimg = cv::Mat::zeros(h, w, CV_32F), dmap = cv::Mat::zeros(out_size.height, out_size.width, CV_64F), x1, x2;
    int32_t refused[4] = {0, 0, 0, 0};
    refused[0] = poselib::GetRectifiedImages(fimg, img2, mx1, my1, mx2, my2, t, x1, x2);
    refused[1] = poselib::rectifyImages(img1, fimg, K1, D1, Rect1, K2, D2, Rect2, K1new, x1, x2);
    refused[2] = poselib::GetRectifiedImages(img1, img2, dmap, my1, mx2, my2, t, x1, x2);
    try {
        poselib::initUndistortRectifyMap(K1, D1, Rect1, K1new, out_size, CV_64F, x1, x2);
    } catch (const cv::Exception &) {
        refused[3] = 1;
    }
    if (!x1.empty() || !x2.empty()) refused[3] = 0;
    std::fwrite(refused, 4, 4, o);
    std::fclose(o);
    return 0;
}

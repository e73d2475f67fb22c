// triang_pts3d_facade.cpp -- poselib::triangPts3D through the C++ drop-in (tests/test_gpu_triang_pts3d.py runs it).
// argv[1]: input file {int32 n; double dist; double R[9], t[3]; double p1[n][2], p2[n][2]; uint8 mask[n]};
// argv[2]: output file:
//   the normal case          {int32 ret; double Q[n][3]; uint8 mask[n]}
//   an empty point set       {int32 ret; int32 mask_cols; int32 Q_empty}        (the one-entry mask passed along stays as it was)
//   Q3D not requested        {int32 ret; uint8 mask[n]}                         (the mask is updated before the call returns -1)
//   no mask, default dist    {int32 ret; double Q[n][3]}
#include <cstdint>
#include <cstdio>

#include "matchinglib_poselib/pose_estim.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    double dist = 0;
    cv::Mat R(3, 3, CV_64F), t(3, 1, CV_64F);
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&dist, 8, 1, f) != 1 || std::fread(R.data, 8, 9, f) != 9 || std::fread(t.data, 8, 3, f) != 3 || n < 1)
        return 2;
    cv::Mat p1(n, 2, CV_64F), p2(n, 2, CV_64F), m0(1, n, CV_8U);
    if (std::fread(p1.data, 16, n, f) != (size_t)n || std::fread(p2.data, 16, n, f) != (size_t)n || std::fread(m0.data, 1, n, f) != (size_t)n) return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    {
        cv::Mat Q, mask = m0.clone();
        const int32_t ret = poselib::triangPts3D(R, t, p1, p2, Q, mask, dist);
        if (Q.rows != n || Q.cols != 3 || Q.type() != CV_64F) return 3;
        std::fwrite(&ret, 4, 1, o);
        std::fwrite(Q.data, 24, n, o);
        std::fwrite(mask.data, 1, n, o);
    }
    {
        cv::Mat e1(0, 2, CV_64F), e2(0, 2, CV_64F), Q, mask(1, 1, CV_8U);
        mask.at<uint8_t>(0, 0) = 7;
        const int32_t ret = poselib::triangPts3D(R, t, e1, e2, Q, mask, dist);
        const int32_t cols = mask.cols == 1 && mask.at<uint8_t>(0, 0) == 7 ? 1 : -1, q_empty = Q.empty() ? 1 : 0;
        std::fwrite(&ret, 4, 1, o);
        std::fwrite(&cols, 4, 1, o);
        std::fwrite(&q_empty, 4, 1, o);
    }
    {
        cv::Mat mask = m0.clone();
        const int32_t ret = poselib::triangPts3D(R, t, p1, p2, cv::noArray(), mask, dist);
        std::fwrite(&ret, 4, 1, o);
        std::fwrite(mask.data, 1, n, o);
    }
    {
        cv::Mat Q;
        const int32_t ret = poselib::triangPts3D(R, t, p1, p2, Q);
        std::fwrite(&ret, 4, 1, o);
        std::fwrite(Q.data, 24, n, o);
    }
    std::fclose(o);
    return 0;
}

// bundle_adjust_facade.cpp -- poselib::refineStereoBA through the C++ drop-in (tests/test_gpu_bundle_adjust.py runs it).
// argv[1]: input file {int32 n; double K1[9], K2[9], R[9], t[3]; double p1[n][2], p2[n][2], Q[n][3]; uint8 mask[n]};
// argv[2]: output file: one record {int32 ret; double R[9], t[3], Q[n][3]} per call --
//   the call with the defaults and the mask; the same without a mask;
//   then the refused options in the order pointsInImgCoords, optimFocalOnly, optimMotionOnly, fixCamMat, dist1 / dist2;
//   then mismatched row counts (p2 one row short) and an empty point set {int32 ret} each.
#include <cstdint>
#include <cstdio>

#include "matchinglib_poselib/pose_estim.h"

static void record(FILE *o, int32_t ret, const cv::Mat &R, const cv::Mat &t, const cv::Mat &Q) {
    std::fwrite(&ret, 4, 1, o);
    std::fwrite(R.data, 8, 9, o);
    std::fwrite(t.data, 8, 3, o);
    std::fwrite(Q.data, 24, (size_t)Q.rows, o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    cv::Mat K1(3, 3, CV_64F), K2(3, 3, CV_64F), R0(3, 3, CV_64F), t0(3, 1, CV_64F);
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(K1.data, 8, 9, f) != 9 || std::fread(K2.data, 8, 9, f) != 9 || std::fread(R0.data, 8, 9, f) != 9 ||
        std::fread(t0.data, 8, 3, f) != 3 || n < 1)
        return 2;
    cv::Mat p1(n, 2, CV_64F), p2(n, 2, CV_64F), Q0(n, 3, CV_64F), mask(1, n, CV_8U);
    if (std::fread(p1.data, 16, n, f) != (size_t)n || std::fread(p2.data, 16, n, f) != (size_t)n || std::fread(Q0.data, 24, n, f) != (size_t)n ||
        std::fread(mask.data, 1, n, f) != (size_t)n)
        return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    {
        cv::Mat R = R0.clone(), t = t0.clone(), Q = Q0.clone();
        const int32_t ret = poselib::refineStereoBA(p1, p2, R, t, Q, K1, K2, false, mask) ? 1 : 0;
        record(o, ret, R, t, Q);
    }
    {
        cv::Mat R = R0.clone(), t = t0.clone(), Q = Q0.clone();
        const int32_t ret = poselib::refineStereoBA(p1, p2, R, t, Q, K1, K2) ? 1 : 0;
        record(o, ret, R, t, Q);
    }
    for (int which = 0; which < 5; ++which) {
        cv::Mat R = R0.clone(), t = t0.clone(), Q = Q0.clone(), d1 = cv::Mat::zeros(1, 5, CV_64F), d2 = cv::Mat::zeros(1, 5, CV_64F);
        bool ret;
        if (which < 4)
            ret = poselib::refineStereoBA(p1, p2, R, t, Q, K1, K2, which == 0, mask, 1.25, 0.05, -1.0, which == 1, which == 2, which == 3);
        else
            ret = poselib::refineStereoBA(p1, p2, R, t, Q, K1, K2, false, mask, 1.25, 0.05, -1.0, false, false, false, d1, d2);
        record(o, ret ? 1 : 0, R, t, Q);
    }
    {
        cv::Mat R = R0.clone(), t = t0.clone(), Q = Q0.clone(), shorter(n - 1, 2, CV_64F, p2.data);
        int32_t ret = poselib::refineStereoBA(p1, shorter, R, t, Q, K1, K2, false, mask) ? 1 : 0;
        std::fwrite(&ret, 4, 1, o);
        cv::Mat e1(0, 2, CV_64F), e2(0, 2, CV_64F), eq(0, 3, CV_64F);
        ret = poselib::refineStereoBA(e1, e2, R, t, eq, K1, K2) ? 1 : 0;
        std::fwrite(&ret, 4, 1, o);
    }
    std::fclose(o);
    return 0;
}

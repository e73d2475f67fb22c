// linear_refine_facade.cpp -- poselib::refineEssentialLinear through the C++ drop-in, called with the reference's signature and defaults
// (tests/test_gpu_linear_refine.py runs it).  argv[1]: input file {int32 n; double th; double p1[n][2], p2[n][2], E[9]; uint8 mask[n]};
// argv[2]: output file, per method of {0x21, 0x23}: {int32 ok; int64 nr_inliers; double E[9]; uint8 mask[n]}, then int32 flags
// {R cleared, t untouched, Kneip returned false, Kneip left E and mask alone}.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "matchinglib_poselib/pose_linear_refinement.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    double th = 0;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&th, 8, 1, f) != 1 || n < 1) return 2;
    cv::Mat p1(n, 2, CV_64F), p2(n, 2, CV_64F), E0(3, 3, CV_64F), m0(1, n, CV_8U);
    if (std::fread(p1.data, 16, n, f) != (size_t)n || std::fread(p2.data, 16, n, f) != (size_t)n || std::fread(E0.data, 8, 9, f) != 9 ||
        std::fread(m0.data, 1, n, f) != (size_t)n)
        return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int method : {poselib::PR_8PT | poselib::PR_PSEUDOHUBER_WEIGHTS, poselib::PR_STEWENIUS | poselib::PR_PSEUDOHUBER_WEIGHTS}) {
        cv::Mat E = E0.clone(), mask = m0.clone();
        size_t nr = 0;
        const int32_t ok = poselib::refineEssentialLinear(p1, p2, E, mask, method, nr, cv::noArray(), cv::noArray(), th) ? 1 : 0;
        const int64_t nr64 = (int64_t)nr;
        std::fwrite(&ok, 4, 1, o);
        std::fwrite(&nr64, 8, 1, o);
        std::fwrite(E.data, 8, 9, o);
        std::fwrite(mask.data, 1, n, o);
    }
    int32_t flags[4] = {0, 0, 0, 0};
    {
        cv::Mat E = E0.clone(), mask = m0.clone(), R = cv::Mat::zeros(3, 3, CV_64F), t = cv::Mat::zeros(3, 1, CV_64F);
        for (int i = 0; i < 3; ++i) R.at<double>(i, i) = 1.0;
        t.at<double>(0, 0) = 1.0;
        size_t nr = 0;
        const bool ok = poselib::refineEssentialLinear(p1, p2, E, mask, 0x21, nr, R, t, th);
        flags[0] = ok && R.empty();
        flags[1] = !t.empty() && t.at<double>(0, 0) == 1.0;
    }
    {
        cv::Mat E = E0.clone(), mask = m0.clone();
        size_t nr = 7;
        flags[2] = !poselib::refineEssentialLinear(p1, p2, E, mask, poselib::PR_KNEIP | poselib::PR_PSEUDOHUBER_WEIGHTS, nr);
        flags[3] = std::memcmp(E.data, E0.data, 72) == 0 && std::memcmp(mask.data, m0.data, n) == 0 && nr == 7;
    }
    std::fwrite(flags, 4, 4, o);
    std::fclose(o);
    return 0;
}

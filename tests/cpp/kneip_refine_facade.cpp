// kneip_refine_facade.cpp -- poselib::refineEssentialLinear with PR_KNEIP through the C++ drop-in (tests/test_gpu_kneip_refine.py runs it).
// argv[1]: input file {int32 n; double th; uint32 seed; double p1[n][2], p2[n][2], E[9]; uint8 mask[n]; double R[9]};
// argv[2]: output file, three records {int32 ok; int64 nr_inliers; double E[9]; uint8 mask[n]; int32 R_empty; double R[9], t[3]}:
//   the call with R and an empty t; the call with R = 2 I (no rotation: the retry path) under setRansacSeed(seed); the same call again.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "matchinglib_poselib/pose_linear_refinement.h"

static void record(FILE *o, bool ok, size_t nr, const cv::Mat &E, const cv::Mat &mask, int n, const cv::Mat &R, const cv::Mat &t) {
    const int32_t ok32 = ok ? 1 : 0, r_empty = R.empty() ? 1 : 0;
    const int64_t nr64 = (int64_t)nr;
    double rt[12] = {0};
    if (!R.empty() && !t.empty()) {
        for (int i = 0; i < 9; ++i) rt[i] = R.at<double>(i / 3, i % 3);
        for (int i = 0; i < 3; ++i) rt[9 + i] = t.at<double>(i, 0);
    }
    std::fwrite(&ok32, 4, 1, o);
    std::fwrite(&nr64, 8, 1, o);
    std::fwrite(E.data, 8, 9, o);
    std::fwrite(mask.data, 1, n, o);
    std::fwrite(&r_empty, 4, 1, o);
    std::fwrite(rt, 8, 12, o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    double th = 0;
    uint32_t seed = 0;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&th, 8, 1, f) != 1 || std::fread(&seed, 4, 1, f) != 1 || n < 1) return 2;
    cv::Mat p1(n, 2, CV_64F), p2(n, 2, CV_64F), E0(3, 3, CV_64F), m0(1, n, CV_8U), R0(3, 3, CV_64F);
    if (std::fread(p1.data, 16, n, f) != (size_t)n || std::fread(p2.data, 16, n, f) != (size_t)n || std::fread(E0.data, 8, 9, f) != 9 ||
        std::fread(m0.data, 1, n, f) != (size_t)n || std::fread(R0.data, 8, 9, f) != 9)
        return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int method = poselib::PR_KNEIP | poselib::PR_PSEUDOHUBER_WEIGHTS;
    {
        cv::Mat E = E0.clone(), mask = m0.clone(), R = R0.clone(), t;
        size_t nr = 0;
        const bool ok = poselib::refineEssentialLinear(p1, p2, E, mask, method, nr, R, t, th);
        record(o, ok, nr, E, mask, n, R, t);
    }
    for (int rep = 0; rep < 2; ++rep) {
        cv::Mat E = E0.clone(), mask = m0.clone(), R = cv::Mat::zeros(3, 3, CV_64F), t = cv::Mat::zeros(3, 1, CV_64F);
        for (int i = 0; i < 3; ++i) R.at<double>(i, i) = 2.0;
        size_t nr = 0;
        poselib::setRansacSeed(seed);
        const bool ok = poselib::refineEssentialLinear(p1, p2, E, mask, method, nr, R, t, th);
        record(o, ok, nr, E, mask, n, R, t);
    }
    std::fclose(o);
    return 0;
}

// homography_pose_facade.cpp -- poselib::estimatePoseHomographies through the C++ drop-in, called with the reference's signature
// (tests/test_gpu_homography_pose_facade.py runs it).  argv[1]: input file {int32 n; double th; double p1[n][2], p2[n][2]; uint8 mask[n]};
// argv[2]: output file, see the writes below.  Every part starts from fresh streams.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "matchinglib_poselib/pose_estim.h"
#include "matchinglib_poselib/pose_homography.h"

static void fresh() { poselib::setArrsacRngState(0xffffffffull, 0xffffffffull); }
static void put_rng(FILE *o) {
    uint64_t st[2];
    poselib::getArrsacRngState(&st[0], &st[1]);
    std::fwrite(st, 8, 2, o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    double th = 0;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&th, 8, 1, f) != 1 || n < 1) return 2;
    cv::Mat p1(n, 2, CV_64F), p2(n, 2, CV_64F), mask_in(1, n, CV_8U);
    if (std::fread(p1.data, 16, n, f) != (size_t)n || std::fread(p2.data, 16, n, f) != (size_t)n || std::fread(mask_in.data, 1, n, f) != (size_t)n) return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    {  // A: every output, vectors that already hold an element (they are ASSIGNED) ->
       //    {int32 rc; double R[9], t[3], E[9]; int32 inliers; uint8 mask[n]; int32 planes; per plane: uint32 num; double strength; double H[9]; int32 rows; streams}
        fresh();
        cv::Mat R, t, E, mask;
        int inliers = -1;
        std::vector<std::pair<cv::Mat, cv::Mat>> pts(1);
        std::vector<unsigned int> num(1, 77u);
        std::vector<cv::Mat> Hs(1, cv::Mat::zeros(1, 1, CV_64F));
        std::vector<double> strength(1, -1.0);
        const int32_t rc = poselib::estimatePoseHomographies(p1, p2, R, t, E, th, inliers, mask, false, false, &pts, &num, &Hs, &strength);
        if (rc != 0 || R.rows != 3 || R.cols != 3 || t.rows != 3 || t.cols != 1 || E.rows != 3 || mask.rows != 1 || mask.cols != n) return 3;
        if (pts.size() != num.size() || Hs.size() != num.size() || strength.size() != num.size()) return 3;
        const int32_t ninl = inliers, planes = (int32_t)num.size();
        std::fwrite(&rc, 4, 1, o), std::fwrite(R.data, 8, 9, o), std::fwrite(t.data, 8, 3, o), std::fwrite(E.data, 8, 9, o);
        std::fwrite(&ninl, 4, 1, o), std::fwrite(mask.data, 1, n, o), std::fwrite(&planes, 4, 1, o);
        for (size_t k = 0; k < num.size(); ++k) {
            const int32_t rows = pts[k].first.rows;
            if (pts[k].second.rows != rows || Hs[k].rows != 3) return 3;
            std::fwrite(&num[k], 4, 1, o), std::fwrite(&strength[k], 8, 1, o), std::fwrite(Hs[k].data, 8, 9, o), std::fwrite(&rows, 4, 1, o);
        }
        put_rng(o);
    }
    {  // B: optional outputs omitted (the reference's defaults) -> {int32 rc; double R[9], t[3]; int32 inliers; streams}
        fresh();
        cv::Mat R, t;
        int inliers = -1;
        const int32_t rc = poselib::estimatePoseHomographies(p1, p2, R, t, cv::noArray(), th, inliers);
        if (rc != 0) return 3;
        const int32_t ninl = inliers;
        std::fwrite(&rc, 4, 1, o), std::fwrite(R.data, 8, 9, o), std::fwrite(t.data, 8, 3, o), std::fwrite(&ninl, 4, 1, o);
        put_rng(o);
    }
    {  // C: without R, without t -> {int32 rc_no_R; int32 t_written; int32 rc_no_t; int32 inliers untouched}
        fresh();
        cv::Mat R, t;
        int inliers = -7;
        const int32_t rc_no_R = poselib::estimatePoseHomographies(p1, p2, cv::noArray(), t, cv::noArray(), th, inliers);
        const int32_t t_written = t.rows == 3 ? 1 : 0;  // the reference writes t before it looks at R
        fresh();
        const int32_t rc_no_t = poselib::estimatePoseHomographies(p1, p2, R, cv::noArray(), cv::noArray(), th, inliers);
        const int32_t untouched = inliers == -7 && R.empty() ? 1 : 0;
        std::fwrite(&rc_no_R, 4, 1, o), std::fwrite(&t_written, 4, 1, o), std::fwrite(&rc_no_t, 4, 1, o), std::fwrite(&untouched, 4, 1, o);
    }
    {  // D: a mask on entry selects the rows; it comes back as the inlier mask over all rows -> {int32 rc; double R[9], t[3]; int32 inliers; uint8 mask[n]; streams}
        fresh();
        cv::Mat R, t, mask = mask_in.clone();
        int inliers = -1;
        const int32_t rc = poselib::estimatePoseHomographies(p1, p2, R, t, cv::noArray(), th, inliers, mask);
        if (rc != 0 || mask.cols != n) return 3;
        const int32_t ninl = inliers;
        std::fwrite(&rc, 4, 1, o), std::fwrite(R.data, 8, 9, o), std::fwrite(t.data, 8, 3, o), std::fwrite(&ninl, 4, 1, o), std::fwrite(mask.data, 1, n, o);
        put_rng(o);
    }
    {  // E: one plane's rows only: -3, outputs untouched -> {int32 rc; int32 untouched}
        fresh();
        cv::Mat q1(n, 2, CV_64F), q2(n, 2, CV_64F);
        for (int i = 0; i < n; ++i)  // every row a copy of a point moved by the same small shift: one plane (a translation), nothing else
            q1.at<double>(i, 0) = p1.at<double>(i, 0), q1.at<double>(i, 1) = p1.at<double>(i, 1), q2.at<double>(i, 0) = p1.at<double>(i, 0) + 0.01,
            q2.at<double>(i, 1) = p1.at<double>(i, 1) - 0.02;
        cv::Mat R, t;
        int inliers = -7;
        const int32_t rc = poselib::estimatePoseHomographies(q1, q2, R, t, cv::noArray(), th, inliers);
        const int32_t untouched = R.empty() && t.empty() && inliers == -7 ? 1 : 0;
        std::fwrite(&rc, 4, 1, o), std::fwrite(&untouched, 4, 1, o);
    }
    std::fclose(o);
    return 0;
}

// ba_multicam_facade.cpp -- poselib::refineMultCamBA through the C++ drop-in (tests/test_gpu_ba_multicam.py runs it).
// argv[1]: input file {int32 m, n; per camera: double K[9], R[9], t[3]; int8 map[n]; int32 k; double ps[k][2]; then double Q[n][3]};
// argv[2]: output file: one record {int32 ret; double R[m][9], t[m][3], Q[n][3]} per call --
//   the defaults; all-ones masks; optimFocalOnly; fixCamMat;
//   then the refused options: pointsInImgCoords, optimMotionOnly, a zero in masks;
//   then the input checks: 14 points, a map whose count disagrees, a map of type CV_8UC1, vectors of differing length.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "matchinglib_poselib/pose_estim.h"

struct Args {
    std::vector<cv::Mat> ps, maps, Rs, ts, Ks;
    cv::Mat Q;
};

static Args clone(const Args &a) {
    Args b;
    for (size_t j = 0; j < a.ps.size(); ++j) {
        b.ps.push_back(a.ps[j].clone());
        b.maps.push_back(a.maps[j].clone());
        b.Rs.push_back(a.Rs[j].clone());
        b.ts.push_back(a.ts[j].clone());
        b.Ks.push_back(a.Ks[j].clone());
    }
    b.Q = a.Q.clone();
    return b;
}

static void record(FILE *o, bool ret, const Args &a) {
    const int32_t r = ret ? 1 : 0;
    std::fwrite(&r, 4, 1, o);
    for (const cv::Mat &R : a.Rs) std::fwrite(R.data, 8, 9, o);
    for (const cv::Mat &t : a.ts) std::fwrite(t.data, 8, 3, o);
    std::fwrite(a.Q.data, 24, (size_t)a.Q.rows, o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t mn[2];
    if (std::fread(mn, 4, 2, f) != 2 || mn[0] < 2 || mn[1] < 15) return 2;
    const int m = mn[0], n = mn[1];
    Args a0;
    for (int j = 0; j < m; ++j) {
        cv::Mat K(3, 3, CV_64F), R(3, 3, CV_64F), t(3, 1, CV_64F), map(1, n, CV_8SC1);
        int32_t k = 0;
        if (std::fread(K.data, 8, 9, f) != 9 || std::fread(R.data, 8, 9, f) != 9 || std::fread(t.data, 8, 3, f) != 3 ||
            std::fread(map.data, 1, n, f) != (size_t)n || std::fread(&k, 4, 1, f) != 1 || k < 0)
            return 2;
        cv::Mat p(k, 2, CV_64F);
        if (k && std::fread(p.data, 16, k, f) != (size_t)k) return 2;
        a0.Ks.push_back(K), a0.Rs.push_back(R), a0.ts.push_back(t), a0.maps.push_back(map), a0.ps.push_back(p);
    }
    a0.Q = cv::Mat(n, 3, CV_64F);
    if (std::fread(a0.Q.data, 24, n, f) != (size_t)n) return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    auto ones_masks = [&](const Args &a) {
        std::vector<cv::Mat> masks;
        for (const cv::Mat &p : a.ps) {
            cv::Mat mk(p.rows, 1, CV_8U);
            for (int i = 0; i < p.rows; ++i) mk.at<unsigned char>(i, 0) = (i & 1) ? 1 : 255;
            masks.push_back(mk);
        }
        return masks;
    };
    {
        Args a = clone(a0);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks), a);
    }
    {
        Args a = clone(a0);
        std::vector<cv::Mat> masks = ones_masks(a);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks, false, masks), a);
    }
    for (int which = 0; which < 2; ++which) {  // optimFocalOnly, fixCamMat: not read in this branch
        Args a = clone(a0);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks, false, cv::noArray(), 1.25, 0.05, -1.0, which == 0, false, which == 1), a);
    }
    {
        Args a = clone(a0);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks, true), a);
    }
    {
        Args a = clone(a0);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks, false, cv::noArray(), 1.25, 0.05, -1.0, false, true), a);
    }
    {
        Args a = clone(a0);
        std::vector<cv::Mat> masks = ones_masks(a);
        masks[1].at<unsigned char>(3, 0) = 0;
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks, false, masks), a);
    }
    {  // 14 points: the first 14 rows of Q and of every map
        Args a = clone(a0);
        cv::Mat Q14(14, 3, CV_64F, a.Q.data);
        std::vector<cv::Mat> maps14;
        for (cv::Mat &mp : a.maps) maps14.push_back(cv::Mat(1, 14, CV_8SC1, mp.data));
        record(o, poselib::refineMultCamBA(a.ps, maps14, a.Rs, a.ts, Q14, a.Ks), a);
    }
    {  // camera 1's map marks one point more than ps[1] holds
        Args a = clone(a0);
        for (int i = 0; i < n; ++i)
            if (!a.maps[1].at<signed char>(0, i)) {
                a.maps[1].at<signed char>(0, i) = 1;
                break;
            }
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks), a);
    }
    {  // the right bytes under the wrong type
        Args a = clone(a0);
        const cv::Mat keep = a.maps[2];  // (owns the bytes the retyped header points at)
        a.maps[2] = cv::Mat(1, n, CV_8UC1, keep.data);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, a.Ks), a);
    }
    {  // one K short
        Args a = clone(a0);
        std::vector<cv::Mat> Ks(a.Ks.begin(), a.Ks.end() - 1);
        record(o, poselib::refineMultCamBA(a.ps, a.maps, a.Rs, a.ts, a.Q, Ks), a);
    }
    std::fclose(o);
    return 0;
}

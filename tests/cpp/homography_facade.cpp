// homography_facade.cpp -- poselib::computeHomographyArrsac / estimateMultHomographys through the C++ drop-in, called with the reference's
// signatures (tests/test_gpu_homography.py runs it).  argv[1]: input file {int32 n; double th; double p1[n][2], p2[n][2]; int32 ne;
// double eth; double e1[ne][2], e2[ne][2]; uint32 minPts}; argv[2]: output file, see the writes below.  The process starts with fresh
// streams; an essential-matrix ARRSAC runs between two homography calls.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "matchinglib_poselib/pose_estim.h"
#include "matchinglib_poselib/pose_homography.h"

static void put_rng(FILE *o) {
    uint64_t st[2];
    poselib::getArrsacRngState(&st[0], &st[1]);
    std::fwrite(st, 8, 2, o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0, ne = 0;
    double th = 0, eth = 0;
    uint32_t min_pts = 4;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&th, 8, 1, f) != 1 || n < 1) return 2;
    cv::Mat p1(n, 2, CV_64F), p2(n, 2, CV_64F);
    if (std::fread(p1.data, 16, n, f) != (size_t)n || std::fread(p2.data, 16, n, f) != (size_t)n) return 2;
    if (std::fread(&ne, 4, 1, f) != 1 || std::fread(&eth, 8, 1, f) != 1 || ne < 1) return 2;
    cv::Mat e1(ne, 2, CV_64F), e2(ne, 2, CV_64F);
    if (std::fread(e1.data, 16, ne, f) != (size_t)ne || std::fread(e2.data, 16, ne, f) != (size_t)ne || std::fread(&min_pts, 4, 1, f) != 1) return 2;
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    {  // A: every output requested -> {int32 ok; double H[9]; uint8 mask[n]; int32 filtered rows; streams}
        cv::Mat H, mask, f1, f2;
        const int32_t ok = poselib::computeHomographyArrsac(p1, p2, H, th, mask, f1, f2) ? 1 : 0;
        if (!ok || mask.cols != n || f1.rows != f2.rows) return 3;
        const int32_t nf = f1.rows;
        std::fwrite(&ok, 4, 1, o), std::fwrite(H.data, 8, 9, o), std::fwrite(mask.data, 1, n, o), std::fwrite(&nf, 4, 1, o);
        put_rng(o);
    }
    {  // B: estimateEssentialMat (ARRSAC, no refinement) on the same streams -> {int32 ok; streams}
        cv::Mat E, mask;
        const int32_t ok = poselib::estimateEssentialMat(E, e1, e2, "ARRSAC", eth, false, mask) ? 1 : 0;
        std::fwrite(&ok, 4, 1, o);
        put_rng(o);
    }
    {  // C: optional outputs omitted -> {int32 ok; double H[9]; streams}
        cv::Mat H;
        const int32_t ok = poselib::computeHomographyArrsac(p1, p2, H, th) ? 1 : 0;
        if (!ok) return 3;
        std::fwrite(&ok, 4, 1, o), std::fwrite(H.data, 8, 9, o);
        put_rng(o);
    }
    {  // D: fresh streams, every output, vectors that already hold one element each ->
       //    {int32 rc; int32 planes; int32 appended (the first elements survived); per plane: uint32 num; double strength; double H[9]; uint8 mask[n]; int32 rows}
        poselib::setArrsacRngState(0xffffffffull, 0xffffffffull);
        std::vector<cv::Mat> masks(1, cv::Mat::zeros(1, 1, CV_8U)), Hs(1, cv::Mat::zeros(1, 1, CV_64F));
        std::vector<std::pair<cv::Mat, cv::Mat>> pts(1);
        std::vector<unsigned int> num(1, 77u);
        std::vector<double> strength(1, -1.0);
        const int32_t rc = poselib::estimateMultHomographys(p1, p2, th, &masks, &pts, &Hs, &num, true, &strength, 0, min_pts);
        const int32_t appended = num.size() > 1 && num[0] == 77u && strength[0] == -1.0 && masks[0].cols == 1 && Hs[0].cols == 1;
        const size_t first = appended ? 1 : 0;
        const int32_t planes = (int32_t)(num.size() - first);
        if (masks.size() != num.size() || Hs.size() != num.size() || pts.size() != num.size() || strength.size() != num.size()) return 3;
        std::fwrite(&rc, 4, 1, o), std::fwrite(&planes, 4, 1, o), std::fwrite(&appended, 4, 1, o);
        for (size_t k = first; k < num.size(); ++k) {
            const int32_t rows = pts[k].first.rows;
            std::fwrite(&num[k], 4, 1, o), std::fwrite(&strength[k], 8, 1, o), std::fwrite(Hs[k].data, 8, 9, o), std::fwrite(masks[k].data, 1, n, o);
            std::fwrite(&rows, 4, 1, o);
        }
        put_rng(o);
    }
    {  // E: fresh streams, one plane at most, only Hs asked for (assigned, not appended) -> {int32 rc; int32 size; double H[9]}
        poselib::setArrsacRngState(0xffffffffull, 0xffffffffull);
        std::vector<cv::Mat> Hs(1, cv::Mat::zeros(1, 1, CV_64F));
        const int32_t rc = poselib::estimateMultHomographys(p1, p2, th, nullptr, nullptr, &Hs, nullptr, true, nullptr, 1, min_pts);
        const int32_t sz = (int32_t)Hs.size();
        if (sz != 1 || Hs[0].cols != 3) return 3;
        std::fwrite(&rc, 4, 1, o), std::fwrite(&sz, 4, 1, o), std::fwrite(Hs[0].data, 8, 9, o);
    }
    {  // F: fresh streams, Hs and masks without num_inl: assigned in the order of discovery -> {int32 rc; int32 size; per plane: double H[9]; uint8 mask[n]}
        poselib::setArrsacRngState(0xffffffffull, 0xffffffffull);
        std::vector<cv::Mat> Hs(1, cv::Mat::zeros(1, 1, CV_64F)), masks(2);
        const int32_t rc = poselib::estimateMultHomographys(p1, p2, th, &masks, nullptr, &Hs, nullptr, true, nullptr, 0, min_pts);
        const int32_t sz = (int32_t)Hs.size();
        if (masks.size() != Hs.size()) return 3;
        std::fwrite(&rc, 4, 1, o), std::fwrite(&sz, 4, 1, o);
        for (int32_t k = 0; k < sz; ++k) std::fwrite(Hs[k].data, 8, 9, o), std::fwrite(masks[k].data, 1, n, o);
    }
    bool threw = false;  // a wrong shape is the reference's CV_Assert
    try {
        cv::Mat H, bad(n, 3, CV_64F);
        poselib::computeHomographyArrsac(bad, p2, H, th);
    } catch (const cv::Exception &) {
        threw = true;
    }
    const int32_t t = threw ? 1 : 0;
    std::fwrite(&t, 4, 1, o);
    std::fclose(o);
    return 0;
}

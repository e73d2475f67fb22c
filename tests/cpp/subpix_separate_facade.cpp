// subpix_separate_facade.cpp -- matchinglib::getSubPixMatches_seperate_Imgs through the C++ drop-in, called with the reference's signature
// (tests/test_gpu_subpix_separate.py runs it and compares with the oracle).
// argv[1]: input file {int32 n1, n2, width1, height1, step1, width2, height2, step2, with_mask; uint8 img1[height1][step1], img2[height2][step2];
//          float kp1[n1][3], kp2[n2][3] (x, y, size)}; the images are handed over as headers onto these rows, so step may exceed width.
// argv[2]: output file {int32 rc; int32 mask_size; uint8 mask[mask_size]; float kp1[n1][2]; float kp2[n2][2]}.
// The mask is handed in holding {true, false, true}; with_mask == 0 passes inliers = NULL and it comes back as it was.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "matchinglib_poselib/matchinglib_matchers.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[9];
    if (std::fread(hd, 4, 9, f) != 9) return 2;
    const int n1 = hd[0], n2 = hd[1];
    std::vector<uint8_t> b1((size_t)hd[3] * hd[4]), b2((size_t)hd[6] * hd[7]);
    std::vector<float> k1((size_t)n1 * 3), k2((size_t)n2 * 3);
    if (std::fread(b1.data(), 1, b1.size(), f) != b1.size() || std::fread(b2.data(), 1, b2.size(), f) != b2.size() ||
        std::fread(k1.data(), 12, n1, f) != (size_t)n1 || std::fread(k2.data(), 12, n2, f) != (size_t)n2)
        return 2;
    std::fclose(f);
    cv::Mat img1(hd[3], hd[2], CV_8U, b1.data(), (size_t)hd[4]), img2(hd[6], hd[5], CV_8U, b2.data(), (size_t)hd[7]);
    std::vector<cv::KeyPoint> kp1((size_t)n1), kp2((size_t)n2);
    for (int i = 0; i < n1; ++i) kp1[i].pt = cv::Point2f(k1[3 * i], k1[3 * i + 1]), kp1[i].size = k1[3 * i + 2];
    for (int i = 0; i < n2; ++i) kp2[i].pt = cv::Point2f(k2[3 * i], k2[3 * i + 1]), kp2[i].size = k2[3 * i + 2];
    std::vector<bool> mask = {true, false, true};
    const int32_t rc = hd[8] ? matchinglib::getSubPixMatches_seperate_Imgs(img1, img2, &kp1, &kp2, &mask) : matchinglib::getSubPixMatches_seperate_Imgs(img1, img2, &kp1, &kp2);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t h[2] = {rc, (int32_t)mask.size()};
    std::fwrite(h, 4, 2, o);
    for (bool b : mask) std::fputc(b ? 1 : 0, o);
    for (const cv::KeyPoint &k : kp1) std::fwrite(&k.pt, 4, 2, o);
    for (const cv::KeyPoint &k : kp2) std::fwrite(&k.pt, 4, 2, o);
    std::fclose(o);
    return 0;
}

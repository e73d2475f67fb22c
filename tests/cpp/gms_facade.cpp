// gms_facade.cpp -- both overloads of filterMatchesGMS through the C++ drop-in, called with the reference's signatures
// (tests/test_gpu_gms.py runs it and compares with the Python path).
// argv[1]: input file {int32 n1, n2, n, width, height, use_scale, use_rotation; float kp1[n1][2], kp2[n2][2]; DMatch matches[n]};
// argv[2]: output file {int32 count_mask; int32 mask_size; uint8 mask[mask_size]; int32 count_list; int32 list_size; DMatch list[list_size]}.
// The mask is handed in holding the three values {true, false, true} and the list holding three default matches: a count of 0 must leave
// the former as it is and empty the latter.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "matchinglib_poselib/gms.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[7];
    if (std::fread(hd, 4, 7, f) != 7) return 2;
    const int n1 = hd[0], n2 = hd[1], n = hd[2];
    std::vector<float> k1((size_t)n1 * 2), k2((size_t)n2 * 2);
    std::vector<cv::DMatch> matches((size_t)n);
    if (std::fread(k1.data(), 8, n1, f) != (size_t)n1 || std::fread(k2.data(), 8, n2, f) != (size_t)n2 ||
        std::fread(matches.data(), sizeof(cv::DMatch), n, f) != (size_t)n)
        return 2;
    std::fclose(f);
    std::vector<cv::KeyPoint> kp1((size_t)n1), kp2((size_t)n2);
    for (int i = 0; i < n1; ++i) kp1[i].pt = cv::Point2f(k1[2 * i], k1[2 * i + 1]);
    for (int i = 0; i < n2; ++i) kp2[i].pt = cv::Point2f(k2[2 * i], k2[2 * i + 1]);
    const cv::Size size(hd[3], hd[4]);
    std::vector<bool> mask = {true, false, true};
    std::vector<cv::DMatch> list(3);
    const int32_t c_mask = filterMatchesGMS(kp1, size, kp2, size, matches, mask, hd[5] != 0, hd[6] != 0);
    const int32_t c_list = filterMatchesGMS(kp1, size, kp2, size, matches, list, hd[5] != 0, hd[6] != 0);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t h1[2] = {c_mask, (int32_t)mask.size()}, h2[2] = {c_list, (int32_t)list.size()};
    std::fwrite(h1, 4, 2, o);
    for (bool b : mask) std::fputc(b ? 1 : 0, o);
    std::fwrite(h2, 4, 2, o);
    if (!list.empty()) std::fwrite(list.data(), sizeof(cv::DMatch), list.size(), o);
    std::fclose(o);
    return 0;
}

// vfc_facade.cpp -- matchinglib::getMatches(VFCrefine = true), filterWithVFC and setVfcSeed through the C++ drop-in, called with the reference's
// signatures (tests/test_gpu_vfc.py runs it and compares with the Python path).
// argv[1]: input file {int32 n1, n2, nbytes; uint32 seed; float kp1[n1][2], kp2[n2][2]; uint8 desc1[n1][nbytes], desc2[n2][nbytes]};
// argv[2]: output file, a sequence of lists {int32 rc; int32 count; DMatch[count]}:
//   per matcher of {LINEAR, BRUTEFORCENMS}: getMatches(VFCrefine = false); getMatches(VFCrefine = true) with setVfcSeed(seed); filterWithVFC on
//   the unfiltered list with the same seed; getMatches(VFCrefine = true) again (reproducibility); the same after clearVfcSeed() (seed 1);
//   at the end filterWithVFC on the first four LINEAR matches (rc -1, empty).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "matchinglib_poselib/matchinglib_matchers.h"
#include "matchinglib_poselib/vfcMatches.h"

static void put(FILE *o, int rc, const std::vector<cv::DMatch> &m) {
    const int32_t h[2] = {rc, (int32_t)m.size()};
    std::fwrite(h, 4, 2, o);
    if (!m.empty()) std::fwrite(m.data(), sizeof(cv::DMatch), m.size(), o);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[3];
    uint32_t seed = 0;
    if (std::fread(hd, 4, 3, f) != 3 || std::fread(&seed, 4, 1, f) != 1) return 2;
    const int n1 = hd[0], n2 = hd[1], nb = hd[2];
    std::vector<float> k1((size_t)n1 * 2), k2((size_t)n2 * 2);
    cv::Mat d1(n1, nb, CV_8U), d2(n2, nb, CV_8U);
    if (std::fread(k1.data(), 8, n1, f) != (size_t)n1 || std::fread(k2.data(), 8, n2, f) != (size_t)n2 ||
        std::fread(d1.data, nb, n1, f) != (size_t)n1 || std::fread(d2.data, nb, n2, f) != (size_t)n2)
        return 2;
    std::fclose(f);
    std::vector<cv::KeyPoint> kp1((size_t)n1), kp2((size_t)n2);
    for (int i = 0; i < n1; ++i) kp1[i].pt = cv::Point2f(k1[2 * i], k1[2 * i + 1]);
    for (int i = 0; i < n2; ++i) kp2[i].pt = cv::Point2f(k2[2 * i], k2[2 * i + 1]);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::vector<cv::DMatch> first;
    for (const char *name : {"LINEAR", "BRUTEFORCENMS"}) {
        std::vector<cv::DMatch> plain, filtered, again, unseeded, direct;
        int rc = matchinglib::getMatches(kp1, kp2, d1, d2, cv::Size(1280, 720), plain, name, false);
        put(o, rc, plain);
        if (first.empty()) first = plain;
        matchinglib::setVfcSeed(seed);
        rc = matchinglib::getMatches(kp1, kp2, d1, d2, cv::Size(1280, 720), filtered, name, true);
        put(o, rc, filtered);
        rc = matchinglib::filterWithVFC(kp1, kp2, plain, direct);
        put(o, rc, direct);
        rc = matchinglib::getMatches(kp1, kp2, d1, d2, cv::Size(1280, 720), again, name, true);
        put(o, rc, again);
        matchinglib::clearVfcSeed();
        rc = matchinglib::getMatches(kp1, kp2, d1, d2, cv::Size(1280, 720), unseeded, name, true);
        put(o, rc, unseeded);
    }
    std::vector<cv::DMatch> four(first.begin(), first.begin() + (first.size() < 4 ? first.size() : 4)), none(3);
    const int rc = matchinglib::filterWithVFC(kp1, kp2, four, none);
    put(o, rc, none);
    std::fclose(o);
    return 0;
}

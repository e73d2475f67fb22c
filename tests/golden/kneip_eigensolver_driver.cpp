// Driver for tests/golden/make_kneip_eigensolver.py: runs opengv::relative_pose::eigensolver of the OpenGV a reference checkout vendors,
// called the way poselib::refineModel calls it for PR_KNEIP (adapter = (bearings of image 2, bearings of image 1), setR12(start), the
// output's rotation preset to the start, all correspondences in order).  Compiled by the generator against that checkout; nothing built
// from it is kept in the repository.
//
// argv[1] = input file, argv[2] = output file, both raw little-endian.
//   in : int32 problems; per problem int32 n, n x 4 doubles (x1 y1 x2 y2, camera coordinates), 9 doubles start rotation (row-major)
//   out: per problem 9 doubles rotation (row-major), 3 doubles translation as OpenGV returns it (not normalised)
#include <cstdint>
#include <cstdio>
#include <vector>

#include <opengv/relative_pose/CentralRelativeAdapter.hpp>
#include <opengv/relative_pose/methods.hpp>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t problems = 0;
    if (std::fread(&problems, 4, 1, in) != 1) return 3;
    for (int32_t p = 0; p < problems; ++p) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, in) != 1 || n < 5) return 3;
        std::vector<double> pts((size_t)n * 4);
        double r0[9];
        if (std::fread(pts.data(), 8, pts.size(), in) != pts.size() || std::fread(r0, 8, 9, in) != 9) return 3;
        opengv::bearingVectors_t b1, b2;
        std::vector<int> idx;
        for (int i = 0; i < n; ++i) {
            opengv::point_t a, b;
            a << pts[4 * i], pts[4 * i + 1], 1.0;
            b << pts[4 * i + 2], pts[4 * i + 3], 1.0;
            a = a / a.norm();
            b = b / b.norm();
            b1.push_back(a);
            b2.push_back(b);
            idx.push_back(i);
        }
        opengv::relative_pose::CentralRelativeAdapter adapter(b2, b1);
        opengv::rotation_t R0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R0(r, c) = r0[3 * r + c];
        adapter.setR12(R0);
        opengv::eigensolverOutput_t eo;
        eo.rotation = R0;
        const opengv::rotation_t R = opengv::relative_pose::eigensolver(adapter, idx, eo);
        double res[12];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) res[3 * r + c] = R(r, c);
        for (int k = 0; k < 3; ++k) res[9 + k] = eo.translation[k];
        if (std::fwrite(res, 8, 12, out) != 12) return 4;
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}

// pose_homography.cpp -- poselib::estimatePoseHomographies / computeHomographyArrsac / estimateMultHomographys
// (P/source/pose_homography.cpp:127-555) over mlpl_pose_homographies / mlpl_homography_arrsac / mlpl_mult_homographies.  Host glue only: the reference's argument checks, cv::Mat <-> pointer plumbing, its
// output behaviour (assign or append), and the process-wide stream pair shared with estimateEssentialMat.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "matchinglib_poselib/pose_homography.h"
#include "facade_internal.h"
#include "mlpl_c.h"

namespace poselib {

namespace {
void flatten(const cv::Mat &P, std::vector<double> &out) {
    out.resize((size_t)P.rows * 2);
    for (int i = 0; i < P.rows; ++i) out[2 * i] = P.at<double>(i, 0), out[2 * i + 1] = P.at<double>(i, 1);
}
cv::Mat rows_of(const std::vector<double> &p, const uint8_t *mask, int n) {
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += mask[i] ? 1 : 0;
    cv::Mat m(cnt, 2, CV_64F);
    for (int i = 0, k = 0; i < n; ++i)
        if (mask[i]) m.at<double>(k, 0) = p[2 * i], m.at<double>(k, 1) = p[2 * i + 1], ++k;
    return m;
}
}  // namespace

bool computeHomographyArrsac(cv::InputArray points1, cv::InputArray points2, cv::OutputArray H, double th, cv::OutputArray mask,
                             cv::OutputArray p_filtered1, cv::OutputArray p_filtered2) {
    // :482-484 (n x 1 CV_64FC2 there; its single-channel view here)
    CV_Assert(points1.cols() == 2 && points1.cols() == points2.cols() && points1.rows() == points2.rows() && points1.type() == CV_64F &&
              points2.type() == CV_64F);
    const int n = points1.rows();
    if (n < 4) return false;
    std::vector<double> a, b;
    flatten(points1.getMat(), a), flatten(points2.getMat(), b);
    std::vector<uint8_t> m((size_t)n);
    double Hv[9];
    int ninl = 0, rc;
    {
        mlpl_facade_arrsac_rng_lock lock;
        rc = mlpl_homography_arrsac(mlpl_facade_default_ctx(), a.data(), b.data(), n, th, lock.state, Hv, m.data(), &ninl, nullptr);
    }
    if (rc == MLPL_E_FAILED) return false;
    if (rc != MLPL_OK) throw cv::Exception(std::string("computeHomographyArrsac: ") + mlpl_last_error());
    if (p_filtered1.needed() && p_filtered2.needed()) {
        p_filtered1.getMatRef() = rows_of(a, m.data(), n);
        p_filtered2.getMatRef() = rows_of(b, m.data(), n);
    }
    if (mask.needed()) {
        mask.create(1, n, CV_8U);
        cv::Mat mm = mask.getMat();
        for (int i = 0; i < n; ++i) mm.at<uint8_t>(0, i) = m[i];
    }
    H.create(3, 3, CV_64F);
    cv::Mat Hm = H.getMat();
    for (int i = 0; i < 9; ++i) Hm.at<double>(i / 3, i % 3) = Hv[i];
    return true;
}

int estimateMultHomographys(cv::InputArray p1, cv::InputArray p2, double th, std::vector<cv::Mat> *inl_mask,
                            std::vector<std::pair<cv::Mat, cv::Mat>> *inl_points, std::vector<cv::Mat> *Hs, std::vector<unsigned int> *num_inl,
                            bool varTh, std::vector<double> *planeStrength, unsigned int maxPlanes, unsigned int minPtsPerPlane) {
    const int n = p1.rows();
    CV_Assert(n == p2.rows() && p1.cols() == 2 && p2.cols() == 2 && n > 3 && p1.type() == CV_64F && p2.type() == CV_64F);  // :318
    std::vector<double> a, b;
    flatten(p1.getMat(), a), flatten(p2.getMat(), b);
    // a plane holds at least max(minPtsPerPlane, 1) correspondences of its own: at most n / that + 1 planes.  The inlier sets are disjoint,
    // so one label per correspondence comes back instead of a mask per possible plane.
    int cap = n / (int)std::max(1u, std::min(minPtsPerPlane, (unsigned)n)) + 1;
    if (maxPlanes && maxPlanes < (unsigned)cap) cap = (int)maxPlanes;
    std::vector<double> Hv((size_t)cap * 9), strength((size_t)cap), th_used((size_t)cap);
    std::vector<int32_t> num((size_t)cap), found_at((size_t)cap), labels((size_t)n, -1);
    const bool want_masks = inl_mask || inl_points;
    int n_planes = 0, rc;
    {
        mlpl_facade_arrsac_rng_lock lock;
        rc = mlpl_mult_homographies_labels(mlpl_facade_default_ctx(), a.data(), b.data(), n, th, varTh ? 1 : 0, maxPlanes, minPtsPerPlane, lock.state,
                                           cap, &n_planes, Hv.data(), num.data(), strength.data(), th_used.data(), found_at.data(),
                                           want_masks ? labels.data() : nullptr, nullptr);
    }
    if (rc != MLPL_OK) throw cv::Exception(std::string("estimateMultHomographys: ") + mlpl_last_error());
    if (n_planes < 0) return -1;
    // :413-460: with num_inl and more than one plane the results are sorted by inlier count (the library's order) and APPENDED; otherwise
    // they are assigned in the order of discovery
    const bool append = num_inl && n_planes > 1;
    std::vector<int> order((size_t)n_planes);
    for (int k = 0; k < n_planes; ++k) order[k] = k;
    if (!append) std::sort(order.begin(), order.end(), [&](int x, int y) { return found_at[x] < found_at[y]; });
    std::vector<std::vector<uint8_t>> masks(want_masks ? (size_t)n_planes : 0, std::vector<uint8_t>((size_t)n, 0));
    if (want_masks)
        for (int j = 0; j < n; ++j)
            if (labels[j] >= 0 && labels[j] < n_planes) masks[(size_t)labels[j]][j] = 1;
    auto put = [&](auto *vec, auto make) {
        if (!vec) return;
        if (!append) vec->clear();
        for (int k = 0; k < n_planes; ++k) vec->push_back(make(order[k]));
    };
    put(inl_mask, [&](int k) {
        cv::Mat m(1, n, CV_8U);
        std::memcpy(m.data, masks[(size_t)k].data(), (size_t)n);
        return m;
    });
    put(inl_points, [&](int k) { return std::make_pair(rows_of(a, masks[(size_t)k].data(), n), rows_of(b, masks[(size_t)k].data(), n)); });
    put(Hs, [&](int k) {
        cv::Mat m(3, 3, CV_64F);
        std::memcpy(m.data, Hv.data() + 9 * (size_t)k, 72);
        return m;
    });
    put(num_inl, [&](int k) { return (unsigned int)num[k]; });
    put(planeStrength, [&](int k) { return strength[k]; });
    return 0;
}

int estimatePoseHomographies(cv::InputArray p1, cv::InputArray p2, cv::OutputArray R, cv::OutputArray t, cv::OutputArray E, double th, int &inliers,
                             cv::InputOutputArray mask, bool checkPlaneStrength, bool varTh, std::vector<std::pair<cv::Mat, cv::Mat>> *inlier_points,
                             std::vector<unsigned int> *numbersHinliers, std::vector<cv::Mat> *homographies, std::vector<double> *planeStrengths) {
    const int n = p1.rows();
    CV_Assert(n == p2.rows() && n > 0 && p1.cols() == 2 && p2.cols() == 2 && p1.type() == CV_64F && p2.type() == CV_64F);
    std::vector<double> a, b;
    flatten(p1.getMat(), a), flatten(p2.getMat(), b);
    std::vector<uint8_t> m_in, m_out((size_t)n);
    if (!mask.empty()) {  // :153-164: a non-empty mask selects the rows the planes are searched in
        cv::Mat mm = mask.getMat();
        CV_Assert(mm.type() == CV_8U && mm.rows * mm.cols == n);
        m_in.assign(mm.data, mm.data + n);
    }
    constexpr int cap = 50;  // MAX_PLANES_PER_PAIR
    double Rv[9], tv[3], Ev[9], Hv[cap * 9], strength[cap];
    int32_t num[cap];
    std::vector<int32_t> labels((size_t)n, -1);
    int result = 0, ninl = 0, n_planes = 0, rc;
    {
        mlpl_facade_arrsac_rng_lock lock;
        rc = mlpl_pose_homographies(mlpl_facade_default_ctx(), a.data(), b.data(), n, m_in.empty() ? nullptr : m_in.data(), th, checkPlaneStrength ? 1 : 0,
                                    varTh ? 1 : 0, lock.state, &result, Rv, tv, Ev, &ninl, m_out.data(), cap, &n_planes, Hv, num, strength,
                                    inlier_points ? labels.data() : nullptr, nullptr);
    }
    if (rc != MLPL_OK) throw cv::Exception(std::string("estimatePoseHomographies: ") + mlpl_last_error());
    if (result != 0) return result;
    if (!t.needed()) return -4;  // :199-207: checked after the alignment, t before R, as in the reference
    t.create(3, 1, CV_64F);
    std::memcpy(t.getMat().data, tv, 24);
    if (!R.needed()) return -4;
    R.create(3, 3, CV_64F);
    std::memcpy(R.getMat().data, Rv, 72);
    if (E.needed()) {
        E.create(3, 3, CV_64F);
        std::memcpy(E.getMat().data, Ev, 72);
    }
    inliers = ninl;
    if (mask.needed()) {
        if (mask.empty()) mask.create(1, n, CV_8U);
        std::memcpy(mask.getMat().data, m_out.data(), (size_t)n);
    }
    if (planeStrengths) planeStrengths->assign(strength, strength + n_planes);
    if (inlier_points) {  // the planes' correspondences among the rows the input mask kept
        std::vector<double> ka, kb;
        for (int i = 0; i < n; ++i)
            if (m_in.empty() || m_in[(size_t)i]) ka.push_back(a[2 * i]), ka.push_back(a[2 * i + 1]), kb.push_back(b[2 * i]), kb.push_back(b[2 * i + 1]);
        const int kept = (int)(ka.size() / 2);
        inlier_points->clear();
        std::vector<uint8_t> sel((size_t)std::max(kept, 1));
        for (int k = 0; k < n_planes; ++k) {
            for (int i = 0; i < kept; ++i) sel[(size_t)i] = labels[(size_t)i] == k;
            inlier_points->push_back(std::make_pair(rows_of(ka, sel.data(), kept), rows_of(kb, sel.data(), kept)));
        }
    }
    if (numbersHinliers) numbersHinliers->assign(num, num + n_planes);
    if (homographies) {
        homographies->clear();
        for (int k = 0; k < n_planes; ++k) {
            cv::Mat h(3, 3, CV_64F);
            std::memcpy(h.data, Hv + 9 * k, 72);
            homographies->push_back(h);
        }
    }
    return 0;
}

}  // namespace poselib

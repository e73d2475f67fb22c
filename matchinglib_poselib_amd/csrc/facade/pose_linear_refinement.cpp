// pose_linear_refinement.cpp -- poselib::refineEssentialLinear (P/source/pose_linear_refinement.cpp:85-309) over mlpl_refine_essential_linear and,
// for PR_KNEIP with R and t requested, mlpl_refine_essential_linear_rt.
// Host glue only: the reference's argument checks, cv::Mat <-> pointer plumbing and its output behaviour.
#include <iostream>
#include <string>
#include <vector>

#include "matchinglib_poselib/pose_linear_refinement.h"
#include "facade_internal.h"
#include "mlpl_c.h"

namespace poselib {

bool refineEssentialLinear(cv::InputArray p1, cv::InputArray p2, cv::InputOutputArray E, cv::InputOutputArray mask, int refineMethod,
                           size_t &nr_inliers, cv::InputOutputArray R, cv::OutputArray t, double th, size_t num_iterative_steps,
                           double threshold_multiplier, double pseudoHuberThreshold_multiplier, double maxRelativeInlierCntLoss) {
    // :99-106
    CV_Assert(p1.rows() == p2.rows() && p1.cols() == 2 && p1.cols() == p2.cols() && p1.rows() == mask.cols() && p1.type() == CV_64F &&
              p1.type() == p2.type() && E.type() == CV_64F && mask.type() == CV_8U);
    const bool kneip = (refineMethod & 0xF) == PR_KNEIP;
    if (kneip && !(R.needed() && t.needed())) {
        // the reference's refineModel gets both pointers whatever the caller passed, but its result can only leave through R and t
        std::cout << "refineEssentialLinear: PR_KNEIP needs R and t! Skipping refinement!" << std::endl;
        return false;
    }
    const cv::Mat P1 = p1.getMat(), P2 = p2.getMat();
    cv::Mat Em = E.getMat(), Mm = mask.getMat();
    CV_Assert(Em.rows == 3 && Em.cols == 3);
    const int n = P1.rows;
    std::vector<double> a((size_t)n * 2), b((size_t)n * 2);
    std::vector<uint8_t> m((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[2 * i] = P1.at<double>(i, 0), a[2 * i + 1] = P1.at<double>(i, 1);
        b[2 * i] = P2.at<double>(i, 0), b[2 * i + 1] = P2.at<double>(i, 1);
        m[i] = Mm.at<uint8_t>(0, i);
    }
    double Ev[9];
    for (int i = 0; i < 9; ++i) Ev[i] = Em.at<double>(i / 3, i % 3);
    int ninl = 0, steps_done = 0;
    if (kneip) {
        // :120-123: R_inout is the passed R, zero when it is empty; the eigensolver's perturbed starts draw from the seed of setRansacSeed
        double Rv[9] = {0}, tv[3] = {0};
        int rt_valid = 0;
        if (!R.empty()) {
            const cv::Mat Rm = R.getMat();
            CV_Assert(Rm.rows == 3 && Rm.cols == 3 && Rm.type() == CV_64F);
            for (int i = 0; i < 9; ++i) Rv[i] = Rm.at<double>(i / 3, i % 3);
            rt_valid = 1;
        }
        const int rc = mlpl_refine_essential_linear_rt(mlpl_facade_default_ctx(), a.data(), b.data(), n, refineMethod, th, (int)num_iterative_steps,
                                                       threshold_multiplier, pseudoHuberThreshold_multiplier, maxRelativeInlierCntLoss, Ev, m.data(),
                                                       &ninl, &steps_done, Rv, tv, &rt_valid, mlpl_facade_draw_seed(), nullptr);
        if (rc == MLPL_E_FAILED) return false;
        if (rc != MLPL_OK) throw cv::Exception(std::string("refineEssentialLinear: ") + mlpl_last_error());
        // :272-293
        if (rt_valid) {
            if (R.empty()) R.create(3, 3, CV_64F);
            if (t.empty()) t.create(3, 1, CV_64F);
            cv::Mat Rm = R.getMat(), tm = t.getMat();
            for (int i = 0; i < 9; ++i) Rm.at<double>(i / 3, i % 3) = Rv[i];
            for (int i = 0; i < 3; ++i) tm.at<double>(i, 0) = tv[i];
        } else {
            R.clear();
        }
        for (int i = 0; i < n; ++i) Mm.at<uint8_t>(0, i) = m[i];
        for (int i = 0; i < 9; ++i) Em.at<double>(i / 3, i % 3) = Ev[i];
        nr_inliers = (size_t)ninl;
        return true;
    }
    const int rc = mlpl_refine_essential_linear(mlpl_facade_default_ctx(), a.data(), b.data(), n, refineMethod, th, (int)num_iterative_steps,
                                                threshold_multiplier, pseudoHuberThreshold_multiplier, maxRelativeInlierCntLoss, Ev, m.data(), &ninl,
                                                &steps_done);
    if (rc == MLPL_E_FAILED) return false;
    if (rc == MLPL_E_BAD_INPUT && (refineMethod & 0xF) == PR_8PT) {
        std::cout << "refineEssentialLinear: PR_8PT needs PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS or PR_NO_WEIGHTS! Skipping refinement!" << std::endl;
        return false;
    }
    if (rc != MLPL_OK) throw cv::Exception(std::string("refineEssentialLinear: ") + mlpl_last_error());
    if (num_iterative_steps > 0 && ((refineMethod & 0xF) == 0 || (refineMethod & 0xF) > PR_KNEIP))
        std::cout << "Refinement algorithm not supported! Skipping!" << std::endl;  // :594-599, printed by the first refit
    // :272-294: none of these solvers yields a rotation or a translation
    if (R.needed()) R.clear();
    else if (t.needed()) t.clear();
    for (int i = 0; i < n; ++i) Mm.at<uint8_t>(0, i) = m[i];
    for (int i = 0; i < 9; ++i) Em.at<double>(i / 3, i % 3) = Ev[i];
    nr_inliers = (size_t)ninl;
    return true;
}

}  // namespace poselib

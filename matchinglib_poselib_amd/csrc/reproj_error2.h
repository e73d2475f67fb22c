// reproj_error2.h -- computeReprojError2 (pose_helper.cpp:639-664) of one correspondence: the ONE copy of the arithmetic behind
// inliers_strict_kernel (pose_prepost.hip) and the hub body of estimatePoseHomographies' final mask (homography_align_impl.h).
#pragma once

namespace mlpl {
__device__ __forceinline__ double reproj_error2_point(const double *__restrict__ E, double x1, double y1, double x2, double y2) {
    const double Ex1_0 = __dadd_rn(__dadd_rn(__dmul_rn(E[0], x1), __dmul_rn(E[1], y1)), E[2]);
    const double Ex1_1 = __dadd_rn(__dadd_rn(__dmul_rn(E[3], x1), __dmul_rn(E[4], y1)), E[5]);
    const double Ex1_2 = __dadd_rn(__dadd_rn(__dmul_rn(E[6], x1), __dmul_rn(E[7], y1)), E[8]);
    const double x2tEx1 = __dadd_rn(__dadd_rn(__dmul_rn(x2, Ex1_0), __dmul_rn(y2, Ex1_1)), Ex1_2);
    const double Etx2_0 = __dadd_rn(__dadd_rn(__dmul_rn(E[0], x2), __dmul_rn(E[3], y2)), E[6]);
    const double Etx2_1 = __dadd_rn(__dadd_rn(__dmul_rn(E[1], x2), __dmul_rn(E[4], y2)), E[7]);
    const double a = __dmul_rn(Ex1_0, Ex1_0), b = __dmul_rn(Ex1_1, Ex1_1), c = __dmul_rn(Etx2_0, Etx2_0), d = __dmul_rn(Etx2_1, Etx2_1);
    return __ddiv_rn(__dmul_rn(x2tEx1, x2tEx1), __dadd_rn(__dadd_rn(__dadd_rn(a, b), c), d));
}
}  // namespace mlpl

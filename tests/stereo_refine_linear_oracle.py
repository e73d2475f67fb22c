"""StereoRefineOracle with the reference's refinement schedule (poselib/source/stereo_pose_refinement.cpp:1429-1722 and :1767-2074): the linear
refinement solvers after the robust estimation (refineMethod, kneipInsteadBA) and on the correspondence pool between robust estimations
(refineMethod_CorrPool, kneipInsteadBA_CorrPool, checkPoolPoseRobust != 1).  TEST INFRASTRUCTURE ONLY.

The refits are linear_refine_oracle.refine_essential_linear and kneip_refine_oracle.refine_essential_linear_rt (seed = the run's seed, as
the drop-in draws it from setRansacSeed), the poses the oracle's recover_pose and triang_pts3d_oracle.triang_pts3d.  Bundle adjustment,
Halign and USAC's Kneip options are not built, so `availableRT` starts false in robust().  `source` is StereoRefine::lastPoseSource().
"""
import numpy as np

import kneip_refine_oracle as KRO
import linear_refine_oracle as LRO
import triang_pts3d_oracle as TPO
from stereo_refine_oracle import Cfg, StereoRefineOracle, AutoThEpiOracle, near_zero

PR_NO_REFINEMENT, PR_STEWENIUS, PR_KNEIP, PR_PSEUDOHUBER_WEIGHTS = 0x0, 0x3, 0x4, 0x20


class LinearCfg(Cfg):
    def __init__(self, **kw):
        self.refineMethod = PR_NO_REFINEMENT
        self.refineMethod_CorrPool = PR_STEWENIUS | PR_PSEUDOHUBER_WEIGHTS
        self.kneipInsteadBA = False
        self.kneipInsteadBA_CorrPool = False
        super().__init__(**kw)

    def linear_ints(self):
        return np.array([self.refineMethod, self.refineMethod_CorrPool, int(self.kneipInsteadBA), int(self.kneipInsteadBA_CorrPool)], np.int32)


def e_from_rt(R, t):  # getEfromRT (pose_helper.cpp:785-788)
    tv = np.asarray(t, np.float64).reshape(-1)
    tv = tv / np.sqrt(np.sum(tv * tv))
    S = np.array([[0, -tv[2], tv[1]], [tv[2], 0, -tv[0]], [-tv[1], tv[0], 0]])
    return S @ R


class StereoRefineLinearOracle(StereoRefineOracle):
    def __init__(self, *a, **kw):
        self.source = 0
        self.log = []    # what the refinement stages did, for the tests
        super().__init__(*a, **kw)

    def check_parameters(self):  # :187-400: nothing forces checkPoolPoseRobust = 1 any more
        c = self.cfg
        if (c.refineMethod_CorrPool & 0xF) == PR_NO_REFINEMENT and not c.refineRTold:
            c.refineMethod_CorrPool = PR_STEWENIUS | PR_PSEUDOHUBER_WEIGHTS
        if c.kneipInsteadBA and (c.refineMethod & 0xF) != PR_KNEIP:
            c.refineMethod = (c.refineMethod & 0xF0) | PR_KNEIP
        if c.kneipInsteadBA_CorrPool and (c.refineMethod_CorrPool & 0xF) != PR_KNEIP:
            c.refineMethod_CorrPool = (c.refineMethod_CorrPool & 0xF0) | PR_KNEIP
        keep = c.checkPoolPoseRobust
        super().check_parameters()
        c.checkPoolPoseRobust = keep
        self.check_tmp = keep

    def add(self, kp1, kp2, dd):
        self.source = 0
        return super().add(kp1, kp2, dd)

    # ---- the two building blocks -------------------------------------------------------------------------------------------------------------
    def linear(self, a, b, E, mask, method, R=None, with_pose=False):
        """refineEssentialLinear(a, b, E, mask, method, nr_inliers_new, R, t, th, 4, 2.0, 0.1, 0.15) -> (ok, E, mask, R, t): E and mask are
        the inputs when it returns false; R, t are None when the call leaves R empty (every solver but Kneip's clears it)."""
        if (method & 0xF) == PR_KNEIP:
            assert with_pose, "the drop-in refuses PR_KNEIP without R and t"
            r = KRO.refine_essential_linear_rt(a, b, E, mask, method, R=R, th=self.th, seed=self.seed)
        else:
            r = LRO.refine_essential_linear(a, b, E, mask, method, th=self.th)
            r = dict(r, rt_valid=False, R=None, t=None)
        self.log.append(("kneip" if (method & 0xF) == PR_KNEIP else "linear", r["rc"] == 0, r.get("steps_done", 0), r.get("attempts_used", 0)))
        if r["rc"] != 0:
            return False, E, mask, R, None
        self.nr_inliers = r["n_inliers"]
        if r["rt_valid"]:
            return True, r["E"], r["mask"], r["R"], r["t"]
        return True, r["E"], r["mask"], None, None

    def triang_with_pose(self, a, b, E, R, t, mask):
        """triangPts3D with a given pose and the plausibility rule (:1566-1577) -> (ok, R, t, Q, mask, source)."""
        o = TPO.triang_pts3d(self.o, R, t, a, b, mask, self.cfg.maxDist3DPtsZ)
        if o["n_good"] < int(np.count_nonzero(mask)) // 3 and o["n_good"] < 100:
            good, R, t, Q, m = self.o.recover_pose(E, a, b, self.cfg.maxDist3DPtsZ, mask)
            return good > 0, R, t, Q, m, 3
        return True, R, t, o["Q"], o["mask"], 2

    def store(self, E, R, t, rebuild, Q, m):
        self.E = e_from_rt(R, t) if rebuild else np.array(E, np.float64).copy()
        self.R, self.t = R, t / np.sqrt(np.sum(t * t))
        self.Q, self.mask_Q = Q, m

    # ---- robustPoseEstimation (:1272-1760) ----------------------------------------------------------------------------------------------------------
    def robust(self, a, b):
        c = self.cfg
        self.Q = self.mask_Q = None
        method, n, auto_th = c.RobMethod, len(a), c.autoTH
        if c.useRANSAC_fewMatches and n < 100:
            method, auto_th = "RANSAC", False
        if auto_th:
            if not hasattr(self, "arrsac_rng"):
                self.arrsac_rng = np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint64)
            auto = AutoThEpiOracle(self.o, self.pix2cam, lambda t: self.o.arrsac_essential(a, b, t, refine=True, rng_state=self.arrsac_rng))
            rc, E, mask, self.th, _ = auto.estimate_e_var_th(a, b, self.th)
            r = dict(ok=(rc == 0), E=E, mask=mask)
        elif method == "RANSAC":
            r = self.o.ransac_essential(a, b, self.th, confidence=0.999, max_iters=1000, lesqu=c.refineRTold, seed=self.seed)
        elif method == "ARRSAC":
            if not hasattr(self, "arrsac_rng"):
                self.arrsac_rng = np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint64)
            r = self.o.arrsac_essential(a, b, self.th, refine=c.refineRTold, rng_state=self.arrsac_rng)
        else:
            r = self.o.lmeds_essential(a, b, confidence=0.999, max_iters=2000, seed=self.seed)
        if not r["ok"]:
            return False
        E, mask = np.array(r["E"], np.float64).copy(), r["mask"].copy()
        self.mask_E = mask.copy()
        self.nr_inliers = int(np.count_nonzero(mask))
        solver = c.refineMethod & 0xF
        rebuild = c.kneipInsteadBA or (solver != PR_NO_REFINEMENT and not c.refineRTold)
        R = t = None
        if c.refineRTold:
            sel = mask.astype(bool)
            _, E, _ = self.o.robust_essential_refine(a[sel], b[sel], E, self.th / 10.0)
        elif solver != PR_NO_REFINEMENT and not c.kneipInsteadBA:
            if solver == PR_KNEIP:   # R passed empty: the perturbed starts
                ok, E, mask, R, t = self.linear(a, b, E, mask, c.refineMethod, None, True)
            else:
                ok, E, mask, _, _ = self.linear(a, b, E, mask, c.refineMethod)
        self.mask_E = mask.copy()
        if R is None:
            good, R, t, Q, m = self.o.recover_pose(E, a, b, c.maxDist3DPtsZ, mask)
            if good <= 0:
                return False
            self.source = 1
        else:
            ok, R, t, Q, m, self.source = self.triang_with_pose(a, b, E, R, t, mask)
            if not ok:
                return False
        use_ba = True
        if c.kneipInsteadBA:   # :1594-1692
            success = False
            ok, E, m, Rn, tn = self.linear(a, b, E, m, c.refineMethod, R, True)
            if ok and Rn is not None:
                self.mask_E = m.copy()
                ok2, Rn, tn, Q, m, _ = self.triang_with_pose(a, b, E, Rn, tn, m)
                if ok2:
                    R, t, use_ba, success, self.source = Rn, tn, False, True, 4
            if not success:
                save = c.refineMethod
                c.refineMethod = PR_STEWENIUS | PR_PSEUDOHUBER_WEIGHTS
                ok, E, m, _, _ = self.linear(a, b, E, m, c.refineMethod)
                if ok:       # (sic) the reference's inverted test: a refinement that succeeds ends the estimation, refineMethod stays changed
                    self.log.append(("kneip_ba_fallback", "refined->fail"))
                    return False
                self.log.append(("kneip_ba_fallback", "not refined->proceed"))
                self.mask_E = m.copy()
                good, R, t, Q, m = self.o.recover_pose(E, a, b, c.maxDist3DPtsZ, m)
                if good <= 0:
                    return False
                self.source = 1
                c.refineMethod = save
        self.store(E, R, t, use_ba and rebuild, Q, m)
        return True

    # ---- refinePoseFromPool (:1767-2074) ---------------------------------------------------------------------------------------------------------------
    def refine_from_pool(self):
        c = self.cfg
        a, b = self.pool_coords()
        n = len(a)
        self.nr_inliers = n
        self.Q = self.mask_Q = None
        E, mask = np.array(self.E, np.float64).copy(), np.ones(n, np.uint8)
        R, t = self.R, self.t
        available = R is not None and t is not None and not near_zero(float(t[0] + t[1] + t[2])) and KRO.is_rotation(R)
        solver = c.refineMethod_CorrPool & 0xF
        if c.refineRTold_CorrPool:
            _, E, _ = self.o.robust_essential_refine(a, b, E, self.th / 10.0)
            available = False
        elif solver != PR_NO_REFINEMENT and not c.kneipInsteadBA_CorrPool:
            if available:
                ok, E, mask, Rn, tn = self.linear(a, b, E, mask, c.refineMethod_CorrPool, R, True)
                if not ok:
                    return False
                if Rn is not None:
                    R, t = Rn, tn
                else:
                    available = False
            elif solver == PR_KNEIP:
                ok, E, mask, Rn, tn = self.linear(a, b, E, mask, c.refineMethod_CorrPool, None, True)
                if ok:
                    if Rn is None:
                        return False
                    R, t, available = Rn, tn, True
            else:
                ok, E, mask, _, _ = self.linear(a, b, E, mask, c.refineMethod_CorrPool)
                if not ok:
                    return False
        self.mask_E = mask.copy()
        if not available:
            good, R, t, Q, m = self.o.recover_pose(E, a, b, c.maxDist3DPtsZ, mask)
            if good <= 0:
                return False
            self.source = 1
        else:
            ok, R, t, Q, m, self.source = self.triang_with_pose(a, b, E, R, t, mask)
            if not ok:
                return False
        use_ba = True
        if c.kneipInsteadBA_CorrPool:   # :1929-2032
            success = False
            ok, E, m, Rn, tn = self.linear(a, b, E, m, c.refineMethod_CorrPool, R, True)
            if ok and Rn is not None:
                before = m.copy()
                ok2, Rn, tn, Q, m, src = self.triang_with_pose(a, b, E, Rn, tn, m)
                if not ok2:
                    return False
                R, t, use_ba, success, self.source = Rn, tn, False, True, 4
                self.mask_E = before
            if not success:
                ok, E, m, _, _ = self.linear(a, b, E, m, PR_STEWENIUS | PR_PSEUDOHUBER_WEIGHTS, R)
                if ok:
                    self.log.append(("kneip_ba_fallback", "refined->fail"))
                    return False
                self.log.append(("kneip_ba_fallback", "not refined->proceed"))
                self.mask_E = m.copy()
                good, R, t, Q, m = self.o.recover_pose(E, a, b, c.maxDist3DPtsZ, m)
                if good <= 0:
                    return False
                self.source = 1
        self.store(E, R, t, use_ba, Q, m)
        return True

// stereo_pose_refinement.h -- drop-in for the reference's poselib::StereoRefine
// (poselib/include/poselib/stereo_pose_refinement.h:100-334, poselib/source/stereo_pose_refinement.cpp).
//
// Built here: the whole multi-frame state machine of addNewCorrespondences() as the reference runs it for the estimators of the hot
// path -- first-call robust initialisation; on later frames the strict getInliers() test against the last pose (GPU), the decision tree
// on the inlier ratios (re-estimate / restore the last pose / re-initialise, :486-560), the correspondence pool with its minPtsDistance
// filter and quality comparison (:2107-2316, :2450-2548), robust re-estimation on the pool (:1075-1128), pose history, the
// near-to-mean pose rating and the stability flags (:2817-3298), maxSkipPairs handling (:3300-3317).
// Every robust estimation and every error evaluation runs on the MI355X (estimateEssentialMat / getPoseTriangPts / mlpl_get_inliers_strict).
//
// The refinement schedule is the reference's: after the robust estimation refineRTold (the estimator's own refinement step plus
// poselib::robustEssentialRefine on the inliers, :1460-1474) or poselib::refineEssentialLinear with refineMethod (:1476-1553), then
// getPoseTriangPts -- or, when Kneip's solver returned the pose itself, poselib::triangPts3D with that pose, falling back to
// getPoseTriangPts when fewer than a third of the inliers and fewer than 100 points triangulate (:1556-1578); kneipInsteadBA runs Kneip's
// solver in the place of bundle adjustment, with the reference's failure path (:1594-1692).  Between robust estimations
// (checkPoolPoseRobust != 1, :680-716) the pool pose is refined by refinePoseFromPool (:1767-2074) with refineRTold_CorrPool,
// refineMethod_CorrPool or kneipInsteadBA_CorrPool in the same way, starting from R_new / t_new.  All of it on the device.
//
// Bundle adjustment of motion and structure (BART = 1, BART_CorrPool = 1: poselib::refineStereoBA on camera coordinates) runs where the
// reference runs it (:1695-1702, :2034-2041), a failure prints "Bundle adjustment failed!" and the estimation goes on, E is rebuilt from R
// and t (:1721, :2052); a failed Kneip-instead-of-BA step goes to bundle adjustment as there (:1650-1658, :1987-1994).
//
// Not built (outside the hot path): homography alignment (Halign), bundle adjustment with the intrinsics in
// the parameter vector (BART = 2, BART_CorrPool = 2) and, inside USAC, Kneip's estimator and refinements.  Consequences:
//   * RobMethod is "USAC" (the reference's default; estimateEssentialOrPoseUSAC with the ConfigUSAC handed to addNewCorrespondences, a
//     degenerate pair -> -2, :1355-1413), "RANSAC", "LMEDS" or "ARRSAC"; Halign makes addNewCorrespondences() return -1; autoTH (ARRSAC
//     with poselib::AutoThEpi's threshold estimation, :1330-1342) is built;
//   * BART / BART_CorrPool = 2 are ignored (reported once on std::cout); where the reference would hand a failed Kneip-instead-of-BA step to
//     that bundle adjustment the library takes the reference's other path, Stewenius with pseudo-Huber weights;
//   * no estimator hands a pose over, so the refinement after the robust estimation never starts from one (`availableRT` starts false,
//     :1429-1449): Kneip's solver there starts from up to 12 perturbed identities drawn from setRansacSeed's seed;
//   * a configuration without a linear refinement keeps the estimator's E as it is, where the reference rebuilds it from R and t
//     (:1721); with one selected E is rebuilt as there;
//   * thinning an over-full pool follows checkPoolSize (:2550-2816): a density image of the pool's left keypoints, elliptic dilate /
//     erode with the reference's border handling, then the weights;
//   * the radius search over the pool returns neighbours by ascending squared distance, as the reference's
//     keyPointTreeInterface::radiusSearch does (nanoflannInterface.cpp:269-300); equal distances come by index.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "matchinglib_poselib/cv_compat.h"
#include "matchinglib_poselib/pose_estim.h"

namespace poselib {

// reference stereo_pose_refinement.h:100-176: every field, the reference's defaults (incl. RobMethod = "USAC").
struct ConfigPoseEstimation {
    ConfigPoseEstimation()
        : dist0_8(nullptr),
          dist1_8(nullptr),
          K0(nullptr),
          K1(nullptr),
          keypointType("FAST"),
          descriptorType("FREAK"),
          th_pix_user(0.8),
          autoTH(false),
          Halign(0),
          RobMethod("USAC"),
          refineMethod(poselib::RefinePostAlg::PR_NO_REFINEMENT),
          refineRTold(false),
          kneipInsteadBA(false),
          BART(0),
          refineMethod_CorrPool(poselib::RefinePostAlg::PR_STEWENIUS | poselib::RefinePostAlg::PR_PSEUDOHUBER_WEIGHTS),
          refineRTold_CorrPool(false),
          kneipInsteadBA_CorrPool(false),
          BART_CorrPool(0),
          verbose(7),
          minStartAggInlRat(0.2),
          relInlRatThLast(0.35),
          relInlRatThNew(0.20),
          minInlierRatSkip(0.38),
          relMinInlierRatSkip(0.7),
          maxSkipPairs(5),
          minInlierRatioReInit(0.6),
          minPtsDistance(3.f),
          maxPoolCorrespondences(30000),
          minContStablePoses(3),
          absThRankingStable(0.075),
          useRANSAC_fewMatches(false),
          checkPoolPoseRobust(3),
          minNormDistStable(0.5),
          raiseSkipCnt(0),
          maxRat3DPtsFar(0.5),
          maxDist3DPtsZ(50.0) {}

    cv::Mat *dist0_8;  // 8 OpenCV-ordered distortion coefficients (CV_64F) of the first / second camera
    cv::Mat *dist1_8;
    cv::Mat *K0;  // 3x3 CV_64F camera matrices
    cv::Mat *K1;
    std::string keypointType;
    std::string descriptorType;
    double th_pix_user;
    bool autoTH;
    int Halign;
    std::string RobMethod;  // USAC, RANSAC, ARRSAC, LMEDS
    int refineMethod;       // enum RefinePostAlg
    bool refineRTold;
    bool kneipInsteadBA;
    int BART;
    int refineMethod_CorrPool;
    bool refineRTold_CorrPool;
    bool kneipInsteadBA_CorrPool;
    int BART_CorrPool;
    int verbose;
    double minStartAggInlRat;
    double relInlRatThLast;
    double relInlRatThNew;
    double minInlierRatSkip;
    double relMinInlierRatSkip;
    size_t maxSkipPairs;
    double minInlierRatioReInit;
    float minPtsDistance;
    size_t maxPoolCorrespondences;
    size_t minContStablePoses;
    double absThRankingStable;
    bool useRANSAC_fewMatches;
    size_t checkPoolPoseRobust;
    double minNormDistStable;
    int raiseSkipCnt;
    double maxRat3DPtsFar;
    double maxDist3DPtsZ;
};

class StereoRefine {
   public:
    // reference stereo_pose_refinement.h:283-291
    cv::Mat E_new;         // newest essential matrix
    cv::Mat Q;             // 3-D points of the latest estimation
    cv::Mat R_new;         // newest rotation
    cv::Mat t_new;         // newest translation (unit norm)
    cv::Mat E_mostLikely;  // pose of the history that is nearest to the centre of gravity of all stored poses
    cv::Mat R_mostLikely;
    cv::Mat t_mostLikely;
    bool poseIsStable = false;
    bool mostLikelyPose_stable = false;

    explicit StereoRefine(ConfigPoseEstimation cfg_pose_, bool verbose_ = false);
    ~StereoRefine();
    void setNewParameters(ConfigPoseEstimation cfg_pose_);
    // 0 ok; -1 robust estimation failed / too few matches / unsupported configuration; -2 the pool had to be re-initialised;
    // -3 too low an inlier ratio after the estimation on the pool (reference codes: stereo_pose_refinement.cpp:411-414).
    int addNewCorrespondences(std::vector<cv::DMatch> matches, std::vector<cv::KeyPoint> kp1, std::vector<cv::KeyPoint> kp2,
                              const poselib::ConfigUSAC &cfg);
    size_t getCorrespondencePoolSize();

    // Read-only views of the private state the reference keeps (same names), for tests and diagnostics.
    double inlierThreshold() const;
    size_t nrInliersNew() const;
    size_t nrCorrsNew() const;
    // where the pose of the last addNewCorrespondences() came from: 0 no pose was computed, 1 getPoseTriangPts, 2 triangPts3D with the pose of
    // Kneip's solver, 3 that triangulation rejected and getPoseTriangPts instead, 4 Kneip's solver instead of bundle adjustment
    int lastPoseSource() const;
    size_t nrEstimations() const;
    size_t skipCounter() const;
    size_t poseHistorySize() const;
    const cv::Mat &maskENew() const;
    // what the last bundle adjustment (BART = 1, BART_CorrPool = 1) was called with, and its verdict; calls counts them since construction
    struct BundleAdjustRecord {
        int calls = 0;
        bool accepted = false;
        cv::Mat p1, p2, R, t, Q, mask;
    };
    const BundleAdjustRecord &lastBundleAdjust() const;

   private:
    struct Impl;
    std::unique_ptr<Impl> d;
};

}  // namespace poselib

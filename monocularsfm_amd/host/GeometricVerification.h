// GeometricVerification.h -- host-side twin of FeatureUtils::FilterMatches
// (src/Feature/FeatureUtils.cpp:176-206): cv::findFundamentalMat(pts1, pts2, FM_RANSAC, 3.0, 0.99,
// mask) on raw pixel coordinates, keep the inliers.  OpenCV's RANSAC (its RNG, its 7-point solver)
// cannot be reproduced bit-for-bit without OpenCV, so this row is OUTSIDE the bit-parity claim
// (SURVEY.md 8a row a13 / 8f-1): same model (fundamental matrix), same error measure (max of the
// two squared point-to-epipolar-line distances), same threshold / confidence / iteration cap,
// deterministic seed; acceptance is inlier-set agreement on data with a true epipolar geometry.
#pragma once
#include <vector>

#include "Types.h"
#include "msfm_match.h"

namespace MonocularSfM {

struct Point2f {
    float x, y;
};

// Returns the inlier mask (1 = keep), one entry per match.  Mirrors findFundamentalMat's cases:
// < 7 points -> no model, empty mask (the caller keeps nothing); exactly 7 -> all ones;
// otherwise RANSAC.
std::vector<unsigned char> FundamentalRansacMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                                 double threshold = 3.0, double confidence = 0.99,
                                                 int max_iters = 1000, unsigned long long seed = 0x5eed5eedULL);

struct CameraIntrinsics {   // pinhole + Brown distortion (the reference's Reconstruction.Camera.* keys)
    double fx, fy, cx, cy, k1, k2, p1, p2;
};

// The calibrated alternative (msfm_emat.h): RANSAC over 5-point essential matrices in normalised coordinates, Sampson
// error <= (threshold / ((fx + fy) / 2))^2, the replayed adaptive stopping rule with sample size 5, no refit.
// < 5 points or a best consensus below 5 -> empty mask (the caller keeps nothing); otherwise a mask of n entries.
// Host twin of the staged device RANSAC (csrc/msfm_verify_e.hip.h): the same bits.
std::vector<unsigned char> EssentialRansacMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                               const CameraIntrinsics& camera, double threshold = 3.0,
                                               double confidence = 0.99, int max_iters = 1000,
                                               unsigned long long seed = 0x5eed5eedULL);

// The planar / rotation-only alternative (msfm_hmat.h): RANSAC over 4-point homographies in pixel coordinates (OpenCV's
// subset check, Hartley-normalised DLT), one-sided reprojection error <= threshold^2, the replayed adaptive stopping rule with
// sample size 4, no refit.  < 4 points or a best consensus below 4 -> empty mask (the caller keeps nothing); otherwise a mask of
// n entries.  Host twin of the staged device RANSAC (csrc/msfm_verify_h.hip.h): the same bits.
std::vector<unsigned char> HomographyRansacMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                                double threshold = 3.0, double confidence = 0.99, int max_iters = 1000,
                                                unsigned long long seed = 0x5eed5eedULL);

// The two-view model selection (msfm_set_model_selection): the epipolar mask of `model` (FundamentalRansacMask, or
// EssentialRansacMask with `camera`) and HomographyRansacMask on the same points; the homography's mask is returned iff
// msfm_select_homography(nE, nH, h_ratio) (csrc/msfm_hostutil.h), else the epipolar one.  *chosen = the model whose mask was returned,
// *n_epipolar / *n_homography = the two masks' counts (any may be NULL).  Host twin of two_view_select_kernel
// (csrc/msfm_verify_select.hip.h): the same bits.
std::vector<unsigned char> TwoViewSelectMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2, int model,
                                             const CameraIntrinsics& camera, double h_ratio, double threshold = 3.0,
                                             double confidence = 0.99, int max_iters = 1000, unsigned long long seed = 0x5eed5eedULL,
                                             int* chosen = nullptr, int* n_epipolar = nullptr, int* n_homography = nullptr);

// The two-view geometry (msfm_set_two_view_geometry, csrc/msfm_pose.h) on top of EssentialRansacMask: the same mask, and in *record
// the relative pose, the triangulation statistics and the reference's test for an initial pair, from the RANSAC's winning E and the
// kept matches in list order (valid = 0 when the mask is empty or no candidate pose puts a match in front of both cameras).  Host
// twin of tv_pose_kernel (csrc/msfm_verify_pose.hip.h): the same bits.
std::vector<unsigned char> TwoViewGeometry(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                           const CameraIntrinsics& camera, const msfm_two_view_params& params,
                                           msfm_two_view_record* record, double threshold = 3.0, double confidence = 0.99,
                                           int max_iters = 1000, unsigned long long seed = 0x5eed5eedULL);

// The two-view pose refinement (msfm_set_two_view_refinement, csrc/msfm_pose_refine.h) behind TwoViewGeometry: (the kept matches'
// normalised undistorted coordinates in list order, the record, the parameters) -> (the record, polished by LM on the Sampson error
// where the refined one stands and untouched otherwise; what the refinement did).  n must be the record's n_kept.  Host twin of
// tv_refine_kernel (csrc/msfm_verify_pose_refine.hip.h): the same bits.
void RefineTwoView(const double* x1, const double* y1, const double* x2, const double* y2, int n, const CameraIntrinsics& camera,
                   const msfm_two_view_params& params, const msfm_two_view_refine_params& refine, msfm_two_view_record* record,
                   msfm_two_view_refinement* refinement);
// what RefineTwoView takes after TwoViewGeometry: x1 | y1 | x2 | y2 of the matches whose mask byte is set, undistorted with `camera`
void KeptNormalised(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2, const std::vector<unsigned char>& mask,
                    const CameraIntrinsics& camera, std::vector<double> kept[4]);

// FeatureUtils::GetAlignedPointsFromMatches + FilterMatches, with the model of SIFTmatch.verification_model
// (msfm_match.h: MSFM_VERIFY_FUNDAMENTAL as the reference, MSFM_VERIFY_ESSENTIAL with `camera`, MSFM_VERIFY_HOMOGRAPHY) and the
// reference's constants.  model_selection (SIFTmatch.model_selection, models 0 and 1 only): TwoViewSelectMask with h_ratio;
// *chosen_model (may be NULL) = the model whose list was kept.
void FilterMatches(const std::vector<KeyPoint>& kpts1, const std::vector<KeyPoint>& kpts2,
                   const std::vector<DMatch>& matches, std::vector<DMatch>* prune_matches,
                   int model = MSFM_VERIFY_FUNDAMENTAL, const CameraIntrinsics& camera = {}, bool model_selection = false,
                   double h_ratio = 0.7, int* chosen_model = nullptr);

}  // namespace MonocularSfM

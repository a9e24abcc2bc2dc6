// FeatureMatching.h -- the reference's matcher classes (include/Feature/FeatureMatching.h:18-130)
// with the same constructor arguments and defaults, running on the gfx950 C ABI
// (include/msfm_match.h).  Differences from the reference, all behind the same interface:
//   * descriptors are uploaded to the GPU once per image instead of being re-read from SQLite
//     for every pair (the "TODO: cache" at src/Feature/FeatureMatching.cpp:31);
//   * the pairs of a whole run are matched as ONE streaming series per GPU (msfm_match_pairs_begin / _next) on device threads,
//     while the calling thread -- the only one that touches SQLite -- writes the rows of the pairs already finished, in the
//     reference's order, groups and transactions (FeatureMatching.cpp:13, 63-72: the reference emits inside its pair loop too).
#pragma once
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "Database.h"
#include "GeometricVerification.h"
#include "Types.h"
#include "msfm_match.h"

namespace MonocularSfM {

class FeatureMatcher {
public:
    FeatureMatcher(const std::string& database_path, const int& max_num_matches = 10240,
                   const double& max_distance = 0.7, const double& distance_ratio = 0.8,
                   const bool& cross_check = true);
    virtual ~FeatureMatcher();

    // FeatureMatching.cpp:10-73: skip pairs that already have a row, match, distance filter,
    // geometric verification, one matches row per pair (rows may be 0), all in one transaction.
    void MatchImagePairs(const std::vector<std::pair<image_t, image_t>>& image_pairs);
    // Any number of such calls at once: what consecutive MatchImagePairs calls would print and write, group by group (one
    // transaction each), while the GPUs are already working on the pairs of the later groups (see FeatureMatching.cpp).
    void MatchImagePairGroups(const std::vector<std::vector<std::pair<image_t, image_t>>>& groups);
    virtual void RunMatching() = 0;

    // FeatureUtils::FilterMatches (F-matrix RANSAC) is applied unless disabled (MSFM_GEOMETRIC_VERIFICATION=0):
    // on the device by default (msfm_match_pairs_verified), by the host twin with MSFM_GEOMETRIC_VERIFICATION=host
    // (GeometricVerification.h; the two give identical lists).
    void SetGeometricVerification(bool on) { geometric_verification_ = on; }
    // SIFTmatch.verification_model: MSFM_VERIFY_FUNDAMENTAL (the default, F as above), MSFM_VERIFY_ESSENTIAL (the essential
    // matrix with the reference's camera) or MSFM_VERIFY_HOMOGRAPHY (planar scenes, rotation-only views; the camera is not read),
    // on every device context (msfm_set_verification_model) or in the host twin (FilterMatches).  Call before RunMatching.
    void SetVerificationModel(int model, const CameraIntrinsics& camera) {
        verification_model_ = model;
        camera_ = camera;
    }
    // SIFTmatch.model_selection / model_selection_h_ratio: under models 0 and 1, every pair also runs the homography and keeps the
    // list msfm_select_homography picks (msfm_set_model_selection on every device context, or TwoViewSelectMask in the host twin).
    // Call before RunMatching.
    // SIFTmatch.two_view_geometry (+ two_view_min_num_inliers / _tri_max_error / _tri_min_angle), model 1 only: every verified pair's
    // msfm_two_view_record (msfm_set_two_view_geometry on every device context, or TwoViewGeometry in the host twin) goes into the
    // two_view_geometries table, in the transaction of the pair's matches row.  Call before RunMatching.
    void SetTwoViewGeometry(bool on, const msfm_two_view_params& params) {
        two_view_geometry_ = on;
        two_view_params_ = params;
    }
    // SIFTmatch.two_view_refine (+ two_view_refine_max_iters / _step_tol / _min_matches), with two_view_geometry only: the records are
    // refined before they are written (msfm_set_two_view_refinement on every device context, or RefineTwoView in the host twin); the
    // table keeps its schema.  Call before RunMatching.
    void SetTwoViewRefinement(bool on, const msfm_two_view_refine_params& params) {
        two_view_refine_ = on;
        two_view_refine_params_ = params;
    }
    // SIFTmatch.tracks (+ tracks_min_num_matches / _min_length / _max_length / _keep_inconsistent): the run's kept matches joined
    // into multi-view tracks (include/msfm_match.h "feature tracks") and written into the `tracks` table, rebuilt whole at the end of
    // the run.  Every device context opens a session over all images in front of the run's matching; rows the run computes are
    // folded on the device as their chunks complete, unless the stored lists are not the device's (host verification, the emission
    // options), in which case the stored rows go through msfm_tracks_add, as do the rows of pairs the exist-check skipped.
    void SetTracks(bool on, int min_num_matches, int min_length, int max_length, bool keep_inconsistent) {
        tracks_ = on;
        tracks_params_ = msfm_track_params{min_num_matches, 0};
        tracks_filter_ = msfm_track_filter{min_length, max_length, keep_inconsistent ? 1 : 0, 0};
    }
    // SIFTmatch.triangulation (+ triangulation_poses / _max_error / _min_angle / _min_views), needs SetTracks: behind the tracks table
    // the kept tracks are triangulated on the first device context under the given poses (msfm_triangulate_tracks) and written into the
    // `points3D` table, rebuilt whole.  A pose of an image the database does not hold ends the run before any matching.
    void SetTriangulation(bool on, const CameraIntrinsics& camera, const std::vector<int32_t>& ids, const std::vector<msfm_pose_rt>& poses,
                          const msfm_triangulation_params& params) {
        triangulation_ = on;
        triangulation_camera_ = msfm_camera{camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2};
        triangulation_ids_ = ids;
        triangulation_poses_ = poses;
        triangulation_params_ = params;
    }
    void SetModelSelection(bool on, double h_ratio) {
        model_selection_ = on;
        h_ratio_ = h_ratio;
    }

protected:
    void OpenDatabaseAndDevice();
    void CloseDatabaseAndDevice();
    void EnsureResident(image_t image_id);
    // every image's descriptors (and keypoints) in ONE table sweep, uploaded straight from SQLite's
    // buffers; uses the optional `descriptors_u8` side table when the database has one.  MSFM_BULK_LOAD=0 falls back
    // to the per-image reads.
    void PreloadAllImages();
    const std::vector<KeyPoint>& KeyPointsOf(image_t image_id);  // read once per image

    std::string database_path_;
    int max_num_matches_;  // stored, never read -- as in the reference
    double max_distance_;
    double distance_ratio_;
    bool cross_check_;
    bool geometric_verification_ = true;
    bool verification_on_host_ = false;  // MSFM_GEOMETRIC_VERIFICATION=host
    bool two_view_refine_ = false;                       // SetTwoViewRefinement
    msfm_two_view_refine_params two_view_refine_params_ = {10, 15, 1e-6};
    bool two_view_geometry_ = false;                     // SetTwoViewGeometry
    msfm_two_view_params two_view_params_ = {100, 0, 2.0, 4.0};
    int verification_model_ = MSFM_VERIFY_FUNDAMENTAL;   // SetVerificationModel
    CameraIntrinsics camera_ = {};                       // (model 1 only)
    bool model_selection_ = false;                       // SetModelSelection
    bool tracks_ = false;                                // SetTracks
    msfm_track_params tracks_params_ = {10, 0};
    msfm_track_filter tracks_filter_ = {2, 0, 0, 0};
    bool tracks_open_ = false;                           // the sessions are open on every device context
    std::vector<int32_t> tracks_ids_;
    bool triangulation_ = false;                         // SetTriangulation
    msfm_camera triangulation_camera_ = {};
    std::vector<int32_t> triangulation_ids_;
    std::vector<msfm_pose_rt> triangulation_poses_;
    msfm_triangulation_params triangulation_params_ = {2.0, 1.5, 2, 0};
    void OpenTrackSessions(bool add_only);
    void FinishTracks();                                 // join the devices' forests, finish, write the table, end the sessions
    double h_ratio_ = 0.7;
    Database* database_ = nullptr;
    // One context per GPU: MSFM_DEVICE (default 0), MSFM_DEVICES="0,1,..." or "all".  The whole descriptor store is replicated on
    // each; the pairs of a run are dealt to the devices in small cost-balanced blocks, round-robin, so that every device's results
    // arrive at the pace the emitter consumes them (SQLite stays on the calling thread).
    struct Device {
        msfm_ctx* ctx = nullptr;
        std::set<image_t> resident;
        std::set<image_t> top_scale;   // images whose top-scale subset lives in the auxiliary slot MSFM_MAX_IMAGES + id
    };
    std::vector<Device> devices_;
    msfm_ctx* ctx_ = nullptr;             // = devices_[0].ctx
    bool bulk_loaded_ = false;
    std::map<image_t, Descriptors> descriptor_cache_;   // host copies, kept only with several devices and without the bulk load
    void EnsureResidentOn(size_t device_index, image_t image_id);
    std::map<image_t, std::vector<KeyPoint>> keypoints_cache_;  // read once per image (verification, pre-emptive filter)
};

class SequentialFeatureMatcher : public FeatureMatcher {
public:
    SequentialFeatureMatcher(const std::string& database_path, const int& overlap = 3,
                             const int& max_num_matches = 10240, const double& max_distance = 0.7,
                             const double& distance_ratio = 0.8, const bool& cross_check = true)
        : FeatureMatcher(database_path, max_num_matches, max_distance, distance_ratio, cross_check),
          overlap_(overlap) {}
    void RunMatching() override;

private:
    int overlap_;
};

class BruteFeatureMatcher : public FeatureMatcher {
public:
    BruteFeatureMatcher(const std::string& database_path, const int& max_pairs_size = 100,
                        const bool& is_preemtive = true, const int& preemtive_num_features = 100,
                        const int& preemtive_min_num_matches = 4, const int& max_num_matches = 10240,
                        const double& max_distance = 0.7, const double& distance_ratio = 0.8,
                        const bool& cross_check = true)
        : FeatureMatcher(database_path, max_num_matches, max_distance, distance_ratio, cross_check),
          max_pairs_size_(max_pairs_size),
          is_preemtive_(is_preemtive),
          preemtive_num_features_(preemtive_num_features),
          preemtive_min_num_matches_(preemtive_min_num_matches) {}
    void RunMatching() override;

private:
    // Wu, "Towards Linear-Time Incremental Structure from Motion", 3DV 2013 (pre-emptive matching)
    std::vector<std::pair<image_t, image_t>> PreemptivelyFilterImagePairs(
        std::vector<std::pair<image_t, image_t>> image_pairs);
    void PreemptivelyFilterGroups(std::vector<std::vector<std::pair<image_t, image_t>>>* groups);
    std::vector<char> PreemptiveKeepFlags(const std::vector<std::pair<image_t, image_t>>& image_pairs);
    int GetTopScaleDescriptors(const image_t& image_id);  // returns the auxiliary store slot (on the first device)
    bool HasTopScaleDescriptorsCache(const image_t& image_id);

    int max_pairs_size_;
    bool is_preemtive_;
    int preemtive_num_features_;
    int preemtive_min_num_matches_;
};

// Matching mode 2 (SIFTmatch.match_type 2, which the reference reserves for "vocabulary tree match" and does not implement): a flat
// visual vocabulary trained on the run's images picks, for every image, its num_nearest_images most similar images
// (msfm_train_vocabulary / msfm_retrieve_pairs on the first device); the union of those pairs is matched in brute mode's orientation,
// order and groups.  Retrieval replaces the pre-emptive filter, which is not applied.
class VocabularyTreeFeatureMatcher : public FeatureMatcher {
public:
    VocabularyTreeFeatureMatcher(const std::string& database_path, const int& num_nearest_images = 50, const int& vocab_num_words = 0,
                                 const int& vocab_train_iters = 0, const int& max_pairs_size = 100, const int& max_num_matches = 10240,
                                 const double& max_distance = 0.7, const double& distance_ratio = 0.8, const bool& cross_check = true)
        : FeatureMatcher(database_path, max_num_matches, max_distance, distance_ratio, cross_check),
          num_nearest_images_(num_nearest_images),
          vocab_num_words_(vocab_num_words),
          vocab_train_iters_(vocab_train_iters),
          max_pairs_size_(max_pairs_size) {}
    void RunMatching() override;

private:
    int num_nearest_images_;
    int vocab_num_words_;     // 0: the library's default (16384)
    int vocab_train_iters_;   // 0: the library's default (8)
    int max_pairs_size_;
};

}  // namespace MonocularSfM

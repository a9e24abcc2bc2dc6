// ComputeMatches.cpp -- drop-in for the reference's `ComputeMatches <config.yaml>` executable
// (sfm/ComputeMatches.cpp:12-68): same argv contract, YAML keys, matcher selection, stdout lines
// and SQLite side effects; the matching itself runs on an MI355X through libmsfm_match.so.
//
// Reference behaviour kept on purpose: SIFTmatch.max_distance / distance_ratio / cross_check are
// parsed but NOT passed to the matcher (sfm/ComputeMatches.cpp:38-42 vs :50,:54), so the
// constructor defaults (0.7 / 0.8 / true) are what run.  MSFM_HONOUR_YAML_MATCH_PARAMS=1 opts
// into using the YAML values instead.
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "FeatureMatching.h"
#include "GeometricVerification.h"
#include "Timer.h"
#include "YamlConfig.h"

using namespace MonocularSfM;

namespace {
// MSFM_CLI_TIMING=1: the wall clock (seconds since the epoch) at which main() was entered and left, on stderr -- against the caller's own
// clock around the process they bound what the loader (before) and the runtimes' exit handlers (after) take
void StampWallClock(const char* what) {
    if (!std::getenv("MSFM_CLI_TIMING")) return;
    const double now = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    std::fprintf(stderr, "[msfm timing] %s at %.6f\n", what, now);
}

// SIFTmatch.triangulation_poses: a text file, '#' starts a comment, every other non-empty line holds 13 numbers:
// image_id r00 r01 r02 r10 r11 r12 r20 r21 r22 tx ty tz  (x_cam = R X + t, R row-major).  False with *error set: unreadable, a line with
// another count of numbers or one that is not a number, a non-finite number, an id that is not an integer in [0, MSFM_MAX_IMAGES) or
// that comes twice.
bool ReadPosesFile(const std::string& path, std::vector<int32_t>* ids, std::vector<msfm_pose_rt>* poses, std::string* error) {
    std::ifstream in(path);
    if (!in) {
        *error = "cannot open " + path;
        return false;
    }
    std::set<int32_t> seen;
    std::string line;
    for (int number = 1; std::getline(in, line); ++number) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.erase(hash);
        std::istringstream fields(line);
        std::vector<double> v;
        std::string word;
        bool bad = false;
        while (fields >> word) {
            char* end = nullptr;
            const double x = std::strtod(word.c_str(), &end);
            if (end == word.c_str() || *end != 0 || !std::isfinite(x)) bad = true;
            v.push_back(x);
        }
        if (v.empty() && !bad) continue;
        const std::string where = path + ":" + std::to_string(number) + ": ";
        if (bad || v.size() != 13) {
            *error = where + "expected 13 finite numbers (image_id r00 .. r22 tx ty tz)";
            return false;
        }
        if (v[0] != std::floor(v[0]) || v[0] < 0 || v[0] >= MSFM_MAX_IMAGES) {
            *error = where + "the image id must be an integer in [0, " + std::to_string(MSFM_MAX_IMAGES) + ")";
            return false;
        }
        const int32_t id = (int32_t)v[0];
        if (!seen.insert(id).second) {
            *error = where + "image " + std::to_string(id) + " is given twice";
            return false;
        }
        msfm_pose_rt pose = {};
        pose.valid = 1;
        for (int k = 0; k < 9; ++k) pose.R[k] = v[(size_t)(1 + k)];
        for (int k = 0; k < 3; ++k) pose.t[k] = v[(size_t)(10 + k)];
        ids->push_back(id);
        poses->push_back(pose);
    }
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    StampWallClock("main entered");
    if (argc != 2) {
        std::cout << "You need specify the YAML file path!" << std::endl;
        exit(-1);
    }
    msfm_host::YamlConfig fs;
    fs.Open(argv[1]);
    if (!fs.isOpened()) {
        std::cout << "YAML file : " << argv[1] << " can't not open!" << std::endl;
        exit(-1);
    }

    std::string database_path;
    int match_type = 1;
    double max_distance = 0.7;
    double distance_ratio = 0.8;
    bool cross_check = true;

    fs.Get("database_path", &database_path);
    fs.Get("SIFTmatch.match_type", &match_type);
    fs.Get("SIFTmatch.max_distance", &max_distance);
    fs.Get("SIFTmatch.distance_ratio", &distance_ratio);
    fs.Get("SIFTmatch.cross_check", &cross_check);

    // (the reference asserts 0 or 1; 2 is the vocabulary mode its configuration reserves, implemented here)
    if (!(match_type == 0 || match_type == 1 || match_type == 2)) {
        std::cerr << "ComputeMatches: SIFTmatch.match_type must be 0 (sequential), 1 (brute) or 2 (vocabulary)" << std::endl;
        std::abort();
    }

    // SIFTmatch.verification_model : 0 (default: the reference's F-matrix check) | 1 (essential matrix with the camera of
    // Reconstruction.Camera.*, the keys the reference's reconstruction reads from the same file; distortion defaults to 0) |
    // 2 (homography, for planar scenes and rotation-only views; no camera)
    int verification_model = 0;
    fs.Get("SIFTmatch.verification_model", &verification_model);
    if (!(verification_model == 0 || verification_model == 1 || verification_model == 2)) {
        std::cerr << "ComputeMatches: SIFTmatch.verification_model must be 0 (fundamental matrix), 1 (essential matrix) or 2 (homography)"
                  << std::endl;
        return EXIT_FAILURE;
    }
    // SIFTmatch.triangulation : 0 (default) | 1 (the tracks' 3-D points under the poses of SIFTmatch.triangulation_poses and the camera
    // of Reconstruction.Camera.*, written into the `points3D` table behind the tracks table; needs SIFTmatch.tracks : 1; optional
    // triangulation_max_error 2.0 px, triangulation_min_angle 1.5 degrees, triangulation_min_views 2; include/msfm_match.h)
    int triangulation = 0;
    fs.Get("SIFTmatch.triangulation", &triangulation);
    if (!(triangulation == 0 || triangulation == 1)) {
        std::cerr << "ComputeMatches: SIFTmatch.triangulation must be 0 or 1" << std::endl;
        return EXIT_FAILURE;
    }
    CameraIntrinsics camera = {0, 0, 0, 0, 0, 0, 0, 0};
    if (verification_model == 1 || triangulation == 1) {
        for (const char* k : {"fx", "fy", "cx", "cy"})
            if (!fs.Has(std::string("Reconstruction.Camera.") + k)) {
                std::cerr << "ComputeMatches: SIFTmatch." << (verification_model == 1 ? "verification_model" : "triangulation")
                          << " : 1 needs Reconstruction.Camera." << k << std::endl;
                return EXIT_FAILURE;
            }
        fs.Get("Reconstruction.Camera.fx", &camera.fx);
        fs.Get("Reconstruction.Camera.fy", &camera.fy);
        fs.Get("Reconstruction.Camera.cx", &camera.cx);
        fs.Get("Reconstruction.Camera.cy", &camera.cy);
        fs.Get("Reconstruction.Camera.k1", &camera.k1);
        fs.Get("Reconstruction.Camera.k2", &camera.k2);
        fs.Get("Reconstruction.Camera.p1", &camera.p1);
        fs.Get("Reconstruction.Camera.p2", &camera.p2);
        const double all[8] = {camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2};
        bool ok = camera.fx > 0 && camera.fy > 0;
        for (double v : all) ok = ok && std::isfinite(v);
        if (!ok) {
            std::cerr << "ComputeMatches: Reconstruction.Camera.* must be finite, with fx, fy > 0" << std::endl;
            return EXIT_FAILURE;
        }
    }

    // SIFTmatch.model_selection : 0 (default) | 1 (under models 0 and 1 every pair also runs the homography and keeps the H list iff
    // nE > 0 and nH >= model_selection_h_ratio * nE -- the reference's Initializer rule, 0.7 by default; include/msfm_match.h)
    int model_selection = 0;
    double h_ratio = 0.7;
    fs.Get("SIFTmatch.model_selection", &model_selection);
    fs.Get("SIFTmatch.model_selection_h_ratio", &h_ratio);
    if (!(model_selection == 0 || model_selection == 1)) {
        std::cerr << "ComputeMatches: SIFTmatch.model_selection must be 0 or 1" << std::endl;
        return EXIT_FAILURE;
    }
    if (model_selection == 1 && verification_model == 2) {
        std::cerr << "ComputeMatches: SIFTmatch.model_selection : 1 chooses between the epipolar model and the homography; it needs "
                     "SIFTmatch.verification_model 0 or 1, not 2"
                  << std::endl;
        return EXIT_FAILURE;
    }
    if (!(std::isfinite(h_ratio) && h_ratio > 0)) {
        std::cerr << "ComputeMatches: SIFTmatch.model_selection_h_ratio must be finite and > 0" << std::endl;
        return EXIT_FAILURE;
    }

    // SIFTmatch.two_view_geometry : 0 (default) | 1 (under verification_model 1 every verified pair also gets a row of the
    // two_view_geometries table: relative pose, triangulation statistics, the reference's test for an initial pair; include/msfm_match.h)
    // SIFTmatch.tracks : 0 (default) | 1 (the run's kept matches joined into multi-view tracks, written into the `tracks` table;
    // tracks_min_num_matches: pairs with fewer matches contribute nothing, default 10 = MapBuilder::Parameters::min_num_matches;
    // tracks_min_length / tracks_max_length (0 = no bound) / tracks_keep_inconsistent: the filter; include/msfm_match.h)
    int tracks = 0, tracks_min_num_matches = 10, tracks_min_length = 2, tracks_max_length = 0, tracks_keep_inconsistent = 0;
    fs.Get("SIFTmatch.tracks", &tracks);
    fs.Get("SIFTmatch.tracks_min_num_matches", &tracks_min_num_matches);
    fs.Get("SIFTmatch.tracks_min_length", &tracks_min_length);
    fs.Get("SIFTmatch.tracks_max_length", &tracks_max_length);
    fs.Get("SIFTmatch.tracks_keep_inconsistent", &tracks_keep_inconsistent);
    if (!(tracks == 0 || tracks == 1) || !(tracks_keep_inconsistent == 0 || tracks_keep_inconsistent == 1) || tracks_min_num_matches < 0 ||
        tracks_max_length < 0) {
        std::cerr << "ComputeMatches: SIFTmatch.tracks and tracks_keep_inconsistent must be 0 or 1, tracks_min_num_matches and "
                     "tracks_max_length must not be negative" << std::endl;
        return EXIT_FAILURE;
    }
    msfm_triangulation_params triangulation_params = {2.0, 1.5, 2, 0};   // Triangulator::Parameters
    std::vector<int32_t> triangulation_ids;
    std::vector<msfm_pose_rt> triangulation_poses;
    if (triangulation == 1) {
        if (tracks != 1) {
            std::cerr << "ComputeMatches: SIFTmatch.triangulation : 1 triangulates the tracks; it needs SIFTmatch.tracks : 1" << std::endl;
            return EXIT_FAILURE;
        }
        std::string poses_path;
        fs.Get("SIFTmatch.triangulation_poses", &poses_path);
        if (!fs.Has("SIFTmatch.triangulation_poses") || poses_path.empty()) {
            std::cerr << "ComputeMatches: SIFTmatch.triangulation : 1 needs SIFTmatch.triangulation_poses : <path>" << std::endl;
            return EXIT_FAILURE;
        }
        fs.Get("SIFTmatch.triangulation_max_error", &triangulation_params.max_error);
        fs.Get("SIFTmatch.triangulation_min_angle", &triangulation_params.min_angle);
        int min_views = triangulation_params.min_views;
        fs.Get("SIFTmatch.triangulation_min_views", &min_views);
        triangulation_params.min_views = min_views;
        if (!(std::isfinite(triangulation_params.max_error) && triangulation_params.max_error >= 0) ||
            !(std::isfinite(triangulation_params.min_angle) && triangulation_params.min_angle >= 0)) {
            std::cerr << "ComputeMatches: SIFTmatch.triangulation_max_error and triangulation_min_angle must be finite and not negative" << std::endl;
            return EXIT_FAILURE;
        }
        std::string error;
        if (!ReadPosesFile(poses_path, &triangulation_ids, &triangulation_poses, &error)) {
            std::cerr << "ComputeMatches: SIFTmatch.triangulation_poses: " << error << std::endl;
            return EXIT_FAILURE;
        }
    }
    int two_view_geometry = 0;
    msfm_two_view_params two_view_params = {100, 0, 2.0, 4.0};
    int two_view_min_num_inliers = two_view_params.min_num_inliers;
    fs.Get("SIFTmatch.two_view_geometry", &two_view_geometry);
    fs.Get("SIFTmatch.two_view_min_num_inliers", &two_view_min_num_inliers);
    fs.Get("SIFTmatch.two_view_tri_max_error", &two_view_params.tri_max_error);
    fs.Get("SIFTmatch.two_view_tri_min_angle", &two_view_params.tri_min_angle);
    two_view_params.min_num_inliers = two_view_min_num_inliers;
    if (!(two_view_geometry == 0 || two_view_geometry == 1)) {
        std::cerr << "ComputeMatches: SIFTmatch.two_view_geometry must be 0 or 1" << std::endl;
        return EXIT_FAILURE;
    }
    if (two_view_geometry == 1 && verification_model != 1) {
        std::cerr << "ComputeMatches: SIFTmatch.two_view_geometry : 1 decomposes the essential matrix; it needs "
                     "SIFTmatch.verification_model : 1"
                  << std::endl;
        return EXIT_FAILURE;
    }
    if (two_view_min_num_inliers < 0 || !(std::isfinite(two_view_params.tri_max_error) && two_view_params.tri_max_error >= 0) ||
        !(std::isfinite(two_view_params.tri_min_angle) && two_view_params.tri_min_angle >= 0)) {
        std::cerr << "ComputeMatches: SIFTmatch.two_view_min_num_inliers, two_view_tri_max_error and two_view_tri_min_angle must be "
                     "finite and not negative"
                  << std::endl;
        return EXIT_FAILURE;
    }
    // SIFTmatch.two_view_refine : 0 (default) | 1 (the pose of every record of the two_view_geometries table is polished over all the
    // pair's kept matches, LM on the Sampson error; two_view_refine_max_iters / _step_tol / _min_matches; include/msfm_match.h)
    int two_view_refine = 0;
    msfm_two_view_refine_params two_view_refine_params = {10, 15, 1e-6};
    int two_view_refine_max_iters = two_view_refine_params.max_iters, two_view_refine_min_matches = two_view_refine_params.min_matches;
    fs.Get("SIFTmatch.two_view_refine", &two_view_refine);
    fs.Get("SIFTmatch.two_view_refine_max_iters", &two_view_refine_max_iters);
    fs.Get("SIFTmatch.two_view_refine_step_tol", &two_view_refine_params.step_tol);
    fs.Get("SIFTmatch.two_view_refine_min_matches", &two_view_refine_min_matches);
    two_view_refine_params.max_iters = two_view_refine_max_iters;
    two_view_refine_params.min_matches = two_view_refine_min_matches;
    if (!(two_view_refine == 0 || two_view_refine == 1)) {
        std::cerr << "ComputeMatches: SIFTmatch.two_view_refine must be 0 or 1" << std::endl;
        return EXIT_FAILURE;
    }
    if (two_view_refine == 1 && two_view_geometry != 1) {
        std::cerr << "ComputeMatches: SIFTmatch.two_view_refine : 1 refines the two-view records; it needs SIFTmatch.two_view_geometry : 1"
                  << std::endl;
        return EXIT_FAILURE;
    }
    // (the optional keys are checked only when the feature is on: a configuration that carries them with it off runs as before)
    if (two_view_refine == 1 && (two_view_refine_max_iters < 1 || two_view_refine_min_matches < 5 ||
                                 !(std::isfinite(two_view_refine_params.step_tol) && two_view_refine_params.step_tol >= 0))) {
        std::cerr << "ComputeMatches: SIFTmatch.two_view_refine_max_iters must be >= 1, two_view_refine_min_matches >= 5, "
                     "two_view_refine_step_tol finite and not negative"
                  << std::endl;
        return EXIT_FAILURE;
    }

    const char* honour = std::getenv("MSFM_HONOUR_YAML_MATCH_PARAMS");
    const bool use_yaml = honour && honour[0] == '1';

    std::unique_ptr<FeatureMatcher> matcher;
    if (match_type == 0) {
        if (use_yaml)
            matcher.reset(new SequentialFeatureMatcher(database_path, 3, 10240, max_distance, distance_ratio, cross_check));
        else
            matcher.reset(new SequentialFeatureMatcher(database_path));
    } else if (match_type == 2) {
        // read only in mode 2: K, and the vocabulary's size and training iterations (0: the library's defaults)
        int num_nearest_images = 50, vocab_num_words = 0, vocab_train_iters = 0;
        fs.Get("SIFTmatch.num_nearest_images", &num_nearest_images);
        fs.Get("SIFTmatch.vocab_num_words", &vocab_num_words);
        fs.Get("SIFTmatch.vocab_train_iters", &vocab_train_iters);
        if (use_yaml)
            matcher.reset(new VocabularyTreeFeatureMatcher(database_path, num_nearest_images, vocab_num_words, vocab_train_iters, 100, 10240,
                                                           max_distance, distance_ratio, cross_check));
        else
            matcher.reset(new VocabularyTreeFeatureMatcher(database_path, num_nearest_images, vocab_num_words, vocab_train_iters));
    } else {
        if (use_yaml)
            matcher.reset(new BruteFeatureMatcher(database_path, 100, true, 100, 4, 10240, max_distance, distance_ratio, cross_check));
        else
            matcher.reset(new BruteFeatureMatcher(database_path));
    }

    matcher->SetVerificationModel(verification_model, camera);
    matcher->SetModelSelection(model_selection == 1, h_ratio);
    matcher->SetTwoViewGeometry(two_view_geometry == 1, two_view_params);
    matcher->SetTwoViewRefinement(two_view_refine == 1, two_view_refine_params);
    matcher->SetTracks(tracks == 1, tracks_min_num_matches, tracks_min_length, tracks_max_length, tracks_keep_inconsistent == 1);
    matcher->SetTriangulation(triangulation == 1, camera, triangulation_ids, triangulation_poses, triangulation_params);

    Timer timer;
    timer.Start();
    matcher->RunMatching();
    timer.PrintMinutes();
    matcher.reset();
    StampWallClock("main left");
    return 0;
}

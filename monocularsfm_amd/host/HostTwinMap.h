// HostTwinMap.h -- test only: the one argument block of the reconstruction stage's host twins (HostTestApi.cpp, twin_triangulate_tracks
// .. twin_map_visibility).  What every twin shares travels in it; a twin's own parameters and outputs follow it as plain arguments.
// tests/twin_host.py mirrors the struct in ctypes and fills it; tests/test_twin_host_abi.py holds the two layouts against each other.
#ifndef MSFM_HOST_TWIN_MAP_H
#define MSFM_HOST_TWIN_MAP_H

#include <stdint.h>

#include "msfm_match.h"

typedef struct host_map {   /* 208 bytes, no implicit padding (pointers are 8 bytes) */
    /* the finished track result, as msfm_fetch_tracks returns it */
    const int64_t* offsets;      /* n_tracks + 1 */
    const int32_t* image_ids;
    const int32_t* point_idx;
    const uint8_t* consistent;   /* may be NULL */
    int64_t n_tracks;
    /* the declared images (any order unless a twin says otherwise); kxy[k] = the (x, y) fp32 pairs of ids[k], NULL for an image
     * without keypoints; kxy itself may be NULL for a twin that reads no pixel */
    const int32_t* ids;
    const float* const* kxy;
    /* the pose list, as msfm_triangulate_tracks takes it */
    const int32_t* pose_ids;
    msfm_pose_rt* poses;
    int32_t n_images;
    int32_t n_poses;
    double cam[8];               /* fx, fy, cx, cy, k1, k2, p1, p2 */
    /* the thresholds of the triangulation that made (or makes) the points */
    double max_error;
    double min_angle;
    int32_t min_views;
    int32_t have_mask;           /* 0: the map-edit twins create the bytes of the computed tracks first */
    /* the slice of a per-track twin: tracks [first, first + count) are computed and written at their own positions, so that several
     * threads can share one state */
    int64_t first;
    int64_t count;
    /* the state: one record per track, one residual and one inlier byte per observation */
    msfm_point3d* points;
    double* residuals;
    uint8_t* mask;               /* may be NULL where a twin only reads it */
} host_map;

#endif

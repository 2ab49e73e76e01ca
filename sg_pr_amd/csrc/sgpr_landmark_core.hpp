// The fusing core of the landmark map: sgpr_landmarks.hip's seven kernels behind one internal
// launcher, for the two entry points that fuse nodes into landmarks - sgpr_landmark_map over every node of a map,
// sgpr_landmark_update over the nodes a map does not explain.  It is not in sgpr_map.hpp: that header holds building
// blocks many files share (§28), this one the launch sequence of one file, declared for one other.
//
// Also here, because both files must form it with the same bits: the map point / live rule of include/sgpr_landmarks.h.
// The constants of the fixed-point sums, the 2^37 limit and the map point itself are sgpr_map_grid.hpp's.
#pragma once
#include "sgpr_internal.hpp"
#include "sgpr_landmarks.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

constexpr int LM_THREADS = NUMBER_THREADS;

// MAP POINT and LIVE of node p of scan g = p / N under poses[g]; `radius` is the table in the kernel's arguments.
// -> live; m = the map point (written whether live or not)
__device__ __forceinline__ bool lm_map_point(const float* centers, const double* poses, const double* radius, int n_labels,
                                             int p, int g, int l, double m[3]) {
#pragma clang fp contract(off)
    const double x = (double)centers[3 * (size_t)p], y = (double)centers[3 * (size_t)p + 1], z = (double)centers[3 * (size_t)p + 2];
    const Se2 X = {poses[4 * (size_t)g], poses[4 * (size_t)g + 1], poses[4 * (size_t)g + 2], poses[4 * (size_t)g + 3]};
    se2_apply(X, x, y, &m[0], &m[1]);
    m[2] = z;
    bool live = l >= 0 && l < n_labels;
    const double r = live ? radius[l] : 0.0;
    return live && r > 0.0 && se2_finite(X) && in_limit37(m[0]) && in_limit37(m[1]) && in_limit37(m[2]);
}

// One fusing job.  The arguments are checked by the caller; G N > 0.
struct LmCoreJob {
    const float* centers;          // [G,N,3]
    const int32_t* labels;         // [G,N] the label array to READ: d_labels, or a masked copy (-1 = takes no part)
    const double* poses;           // [G,4]
    int G, N;
    const int32_t* h_starts;       // session table of the G scans (checked)
    int n_sessions;
    const double* h_radius;
    int n_labels;
    double tau_z;
    int id_base;                   // the id of the first landmark found; records go to [id_base, max_landmarks)
    int first_base;                // lm_first = first_base + the lowest flat node index
    int session_shift;             // session bit = 1 << (session_shift + session(g))
    int max_landmarks;
    double* lm_center;
    int32_t* lm_label;
    int32_t* lm_count;
    int32_t* lm_first;
    uint64_t* lm_sessions;
    double* lm_spread;
    int32_t* node_landmark;        // [G,N] the id of every live node, -1 of any other
    int32_t* num;                  // (id_base + landmarks found, live nodes)
};

size_t lm_core_workspace_bytes(size_t P);

// memset + the seven kernels on `s`; `fn` names the entry point in an error message.  -> SGPR_OK or SGPR_E_HIP
int lm_core_launch(const char* fn, const LmCoreJob& job, void* d_workspace, hipStream_t s);

}  // namespace sgpr

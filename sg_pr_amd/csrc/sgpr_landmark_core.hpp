// The fusing core of the landmark map: sgpr_landmarks.hip's seven kernels behind one internal
// launcher, for the two entry points that fuse nodes into landmarks - sgpr_landmark_map over every node of a map,
// sgpr_landmark_update over the nodes a map does not explain.  It is not in sgpr_map.hpp: that header holds building
// blocks many files share (§28), this one the launch sequence of one file, declared for one other.
//
// Also here, because both files must form them with the same bits: the constants of the fixed-point sums and the map
// point / live rule of include/sgpr_landmarks.h.
#pragma once
#include "sgpr_internal.hpp"
#include "sgpr_landmarks.h"

namespace sgpr {

constexpr int LM_THREADS = 256;
constexpr double LM_FIX = 16777216.0;          // 2^24
constexpr double LM_LIMIT = 137438953472.0;    // 2^37
constexpr double LM_D2_CAP = 1048576.0;        // 2^20

__device__ __forceinline__ bool lm_in_limit(double v) { return isfinite(v) && fabs(v) <= LM_LIMIT; }

// MAP POINT and LIVE of node p of scan g = p / N under poses[g]; `radius` is the table in the kernel's arguments.
// -> live; m = the map point (written whether live or not)
__device__ __forceinline__ bool lm_map_point(const float* centers, const double* poses, const double* radius, int n_labels,
                                             int p, int g, int l, double m[3]) {
#pragma clang fp contract(off)
    const double x = (double)centers[3 * (size_t)p], y = (double)centers[3 * (size_t)p + 1], z = (double)centers[3 * (size_t)p + 2];
    const double c = poses[4 * (size_t)g], s = poses[4 * (size_t)g + 1], X = poses[4 * (size_t)g + 2], Y = poses[4 * (size_t)g + 3];
    m[0] = (c * x - s * y) + X;
    m[1] = (s * x + c * y) + Y;
    m[2] = z;
    bool live = l >= 0 && l < n_labels;
    const double r = live ? radius[l] : 0.0;
    return live && r > 0.0 && isfinite(c) && isfinite(s) && isfinite(X) && isfinite(Y) && lm_in_limit(m[0]) && lm_in_limit(m[1]) &&
           lm_in_limit(m[2]);
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

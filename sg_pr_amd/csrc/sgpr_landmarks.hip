// The semantic landmark map (sgpr_landmark_map; include/sgpr_landmarks.h): every node of every scan of
// a map goes into the map frame, nodes of one label within that label's radius link, and the connected components of
// the link graph are the landmarks.  sgpr_cluster.hip's scheme for one scan's points, across a whole map: a cell table,
// a lock-free union-find whose roots are lowest indices, fixed-point integer sums - here in float64, with a radius per
// label, sessions and spreads.  HBM-bound integer / pointer work, no matrix cores.
//
//   lm_transform_kernel   one thread per node: the map point, live or dead; a live node enters the open-addressing cell
//                         table (key: a hash of (label, ix, iy)) and is pushed on its cell's linked list.
//   lm_union_kernel       one thread per live node: the lower-indexed nodes on the lists of its 9 neighbouring cells are
//                         tested with the header's rule and united.  The larger root is hooked under the smaller by a
//                         CAS, so a component's root is its LOWEST NODE INDEX whatever the execution order.
//   lm_flatten_kernel     the forest is final: every live node finds its root and adds its count, its three fixed-point
//                         coordinates and its session bit to the root (integer atomics: any order, same sums).  Each
//                         workgroup counts its roots and its live nodes.
//   lm_scan_kernel        one workgroup: exclusive prefix sum of the per-workgroup root counts; d_num.
//   lm_record_kernel      the id of a root = roots before it = its workgroup's prefix + its rank inside the workgroup;
//                         records of ids below max_landmarks are written.
//   lm_spread_kernel      second pass: every live node gets its landmark id and adds its capped squared distance to
//                         the centre (recomputed from the root's sums: the same expression, the same bits).
//   lm_finish_kernel      spread of every recorded landmark.
//
// The cell table and the union-find are sgpr_map.hpp's, with their SIZING, VISIBILITY and TERMINATION arguments: the
// table has table_slots(G N) slots and every key in it belongs to some node; the cell lists are complete before the
// kernel that walks them starts; the forest is the only memory another workgroup rewrites while it is read.  The push
// on a cell's list, the linking step of lm_union_kernel, the scan and the rank of the numbering are sgpr_map_grid.hpp's
// (grid_push, link_item, scan_block_counts, rank_in_block), shared with sgpr_landmark_merge.hip.
// Everything else is handed from one kernel to the next on one stream.  No floating-point atomics, no inline assembly,
// plain vector stores.
//
// The launch sequence is lm_core_launch (sgpr_landmark_core.hpp): sgpr_landmark_map runs it on every node of a map,
// sgpr_landmark_update (sgpr_landmark_update.hip) on the nodes its map does not explain, with a masked label array, an
// id base, a `first` base and a session shift; all three are 0 here.
//
// Cells are a linked list per cell; the cell-sorted layout (count, scan, scatter, a wave per cell with the cell in LDS)
// is not built.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_core.hpp"
#include "sgpr_landmarks.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

struct LmWs {
    double* m;                     // [P][3] map point
    int* lab;                      // [P] label of a live node, -1 of a dead one
    int* parent;                   // [P] union-find forest
    int* next;                     // [P] linked list of the node's cell; after flatten: the node's root
    int* cnt;                      // [P] members per root
    int* id;                       // [P] landmark id of a root
    long long* sum;                // [P][3] fixed-point coordinate sums per root
    unsigned long long* q;         // [P] fixed-point sum of squared distances per root
    unsigned long long* sess;      // [P] session mask per root
    unsigned long long* cell_key;  // [H]
    int* cell_head;                // [H]
    int* blk_roots;                // [B] roots per workgroup; after the scan: roots before the workgroup
    int* blk_live;                 // [B] live nodes per workgroup
    unsigned long long hmask;      // H - 1 (H a power of two)
    // (next, cell_key, cell_head, hmask) as the grid the shared steps take
    __device__ __forceinline__ CellGrid grid() const { return CellGrid{next, cell_key, cell_head, hmask}; }
};

struct LmArgs {
    const float* centers;
    const int32_t* labels;
    const double* poses;
    double* lm_center;
    int32_t* lm_label;
    int32_t* lm_count;
    int32_t* lm_first;
    unsigned long long* lm_sessions;
    double* lm_spread;
    int32_t* node_landmark;
    int32_t* num;
    int P, N, n_labels, n_sessions, max_landmarks, B;
    int id_base, first_base, session_shift;
    double tau_z;
    double radius[SGPR_LANDMARK_MAX_LABELS];
    int32_t starts[SGPR_SESSION_MAX];
};

// The cell width of a label, the cell of a coordinate and the key of a cell (lm_cell_width, lm_cell_coord, lm_cell_key)
// are sgpr_map.hpp's, with the proof that two nodes in range are never two cells apart; the map point and the live rule
// (lm_map_point) are sgpr_landmark_core.hpp's.

__global__ __launch_bounds__(LM_THREADS) void lm_transform_kernel(const LmWs w, const LmArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const int l = a.labels[p];
    double m[3];
    const bool live = lm_map_point(a.centers, a.poses, a.radius, a.n_labels, p, p / a.N, l, m);
    const double mx = m[0], my = m[1], mz = m[2];
    w.m[3 * (size_t)p] = mx;
    w.m[3 * (size_t)p + 1] = my;
    w.m[3 * (size_t)p + 2] = mz;
    w.lab[p] = live ? l : -1;
    w.parent[p] = p;
    w.cnt[p] = 0;
    w.id[p] = -1;
    w.sum[3 * (size_t)p] = 0;
    w.sum[3 * (size_t)p + 1] = 0;
    w.sum[3 * (size_t)p + 2] = 0;
    w.q[p] = 0ull;
    w.sess[p] = 0ull;
    if (!live) {
        w.next[p] = -1;
        a.node_landmark[p] = -1;
        return;
    }
    grid_push(w.grid(), p, l, lm_cell_width(a.radius[l]), mx, my);
}

__global__ __launch_bounds__(LM_THREADS) void lm_union_kernel(const LmWs w, const LmArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    if (p >= a.P) return;
    link_item(w.grid(), w.m, w.lab, w.parent, a.radius, a.tau_z, p);
}

// the sum of v over the workgroup, valid in thread 0
__device__ __forceinline__ int lm_block_sum(int v, int* wsum) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < LM_THREADS / 64; ++i) t += wsum[i];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(LM_THREADS) void lm_flatten_kernel(const LmWs w, const LmArgs a) {
    __shared__ int wsum[LM_THREADS / 64];
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    const bool live = p < a.P && w.lab[p] >= 0;
    int root = -1;
    if (live) {
        root = uf_root_final(w.parent, p);
        w.next[p] = root;                                       // (the cell lists are dead) the node's root
        const int g = p / a.N;
        const int sess = session_of(a.starts, a.n_sessions, g);
        atomicAdd(&w.cnt[root], 1);
        for (int k = 0; k < 3; ++k)
            atomicAdd(reinterpret_cast<unsigned long long*>(&w.sum[3 * (size_t)root + k]),
                      (unsigned long long)llrint(w.m[3 * (size_t)p + k] * MAP_FIX));
        atomicOr(&w.sess[root], 1ull << (a.session_shift + sess));
    }
    const int roots = lm_block_sum(live && root == p ? 1 : 0, wsum);
    const int lives = lm_block_sum(live ? 1 : 0, wsum);
    if (threadIdx.x == 0) {
        w.blk_roots[blockIdx.x] = roots;
        w.blk_live[blockIdx.x] = lives;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void lm_scan_kernel(const LmWs w, const LmArgs a) {
    __shared__ int part[SCAN_THREADS];
    __shared__ int live_part[SCAN_THREADS];
    scan_block_counts<true>(w.blk_roots, w.blk_live, a.B, part, live_part);
    if (threadIdx.x == SCAN_THREADS - 1) {
        a.num[0] = a.id_base + part[threadIdx.x];
        a.num[1] = live_part[threadIdx.x];
    }
}

__device__ __forceinline__ double lm_center(const LmWs& w, int root, int k, double cnt) {
    return (double)w.sum[3 * (size_t)root + k] / (cnt * MAP_FIX);
}

__global__ __launch_bounds__(LM_THREADS) void lm_record_kernel(const LmWs w, const LmArgs a) {
    __shared__ int wcount[LM_THREADS / 64];
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    const bool root = p < a.P && w.lab[p] >= 0 && w.next[p] == p;
    const int rank = rank_in_block(root, wcount);
    if (!root) return;
    const int id = a.id_base + w.blk_roots[blockIdx.x] + rank;
    w.id[p] = id;
    if (id >= a.max_landmarks) return;
    const int n = w.cnt[p];
    const double cnt = (double)n;
    for (int k = 0; k < 3; ++k) a.lm_center[3 * (size_t)id + k] = lm_center(w, p, k, cnt);
    a.lm_label[id] = w.lab[p];
    a.lm_count[id] = n;
    a.lm_first[id] = a.first_base + p;
    a.lm_sessions[id] = w.sess[p];
}

__global__ __launch_bounds__(LM_THREADS) void lm_spread_kernel(const LmWs w, const LmArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    if (p >= a.P || w.lab[p] < 0) return;
    const int root = w.next[p];
    a.node_landmark[p] = w.id[root];
    const double cnt = (double)w.cnt[root];
    const double ex = w.m[3 * (size_t)p] - lm_center(w, root, 0, cnt), ey = w.m[3 * (size_t)p + 1] - lm_center(w, root, 1, cnt);
    const double d2 = ex * ex + ey * ey;
    atomicAdd(&w.q[root], (unsigned long long)llrint(fmin(d2, MAP_D2_CAP) * MAP_FIX));
}

__global__ __launch_bounds__(LM_THREADS) void lm_finish_kernel(const LmWs w, const LmArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    if (p >= a.P || w.lab[p] < 0 || w.next[p] != p) return;
    const int id = w.id[p];
    if (id >= a.max_landmarks) return;
    a.lm_spread[id] = sqrt((double)w.q[p] / ((double)w.cnt[p] * MAP_FIX));
}

bool lm_size_ok(int G, int N) { return G >= 0 && N >= 0 && (long long)G * (long long)N <= 0x7fffffffll; }

}  // namespace

size_t lm_core_workspace_bytes(size_t P) {
    const size_t b = (P + LM_THREADS - 1) / LM_THREADS;
    return align256(P * 24) * 2 + align256(P * 4) * 4 + align256(P * 8) * 2 + grid_bytes(P) + align256(b * 4) * 2;
}

int lm_core_launch(const char* fn, const LmCoreJob& job, void* d_workspace, hipStream_t s) {
    const size_t P = (size_t)job.G * (size_t)job.N;
    Carver ws{static_cast<unsigned char*>(d_workspace)};
    LmWs w;
    const size_t H = table_slots(P);
    const int B = (int)((P + LM_THREADS - 1) / LM_THREADS);
    w.hmask = H - 1;
    w.m = ws.take<double>(3 * P);
    w.sum = ws.take<long long>(3 * P);
    w.lab = ws.take<int>(P);
    w.parent = ws.take<int>(P);
    w.next = ws.take<int>(P);
    w.cnt = ws.take<int>(P);
    w.id = ws.take<int>(P);
    w.q = ws.take<unsigned long long>(P);
    w.sess = ws.take<unsigned long long>(P);
    w.cell_key = ws.take<unsigned long long>(H);
    w.cell_head = ws.take<int>(H);
    w.blk_roots = ws.take<int>(B);
    w.blk_live = ws.take<int>(B);

    LmArgs a = {};
    a.centers = job.centers;
    a.labels = job.labels;
    a.poses = job.poses;
    a.lm_center = job.lm_center;
    a.lm_label = job.lm_label;
    a.lm_count = job.lm_count;
    a.lm_first = job.lm_first;
    a.lm_sessions = reinterpret_cast<unsigned long long*>(job.lm_sessions);
    a.lm_spread = job.lm_spread;
    a.node_landmark = job.node_landmark;
    a.num = job.num;
    a.P = (int)P;
    a.N = job.N;
    a.n_labels = job.n_labels;
    a.max_landmarks = job.max_landmarks;
    a.B = B;
    a.id_base = job.id_base;
    a.first_base = job.first_base;
    a.session_shift = job.session_shift;
    a.tau_z = job.tau_z;
    for (int l = 0; l < job.n_labels; ++l) a.radius[l] = job.h_radius[l];
    fill_session_table(a.starts, &a.n_sessions, job.h_starts, job.n_sessions);

    const std::string what = fn;
    // cell_key | cell_head: empty keys, list ends (-1)
    hipError_t e = hipMemsetAsync(w.cell_key, 0xff, grid_clear_bytes(P), s);
    if (e != hipSuccess) return hip_fail(e, (what + ": memset").c_str());
    const dim3 grid(B), block(LM_THREADS);
    hipLaunchKernelGGL(lm_transform_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(lm_union_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(lm_flatten_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(lm_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, w, a);
    hipLaunchKernelGGL(lm_record_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(lm_spread_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(lm_finish_kernel, grid, block, 0, s, w, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, (what + ": launch").c_str());
    return SGPR_OK;
}

}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_workspace_bytes(int G, int N) {
    if (!lm_size_ok(G, N) || G == 0 || N == 0) return 0;
    return lm_core_workspace_bytes((size_t)G * (size_t)N);
}

int sgpr_landmark_map(const float* d_centers, const int32_t* d_labels, int G, int N, const double* d_poses,
                      const int32_t* h_starts, int n_sessions, const double* h_radius, int n_labels, double tau_z,
                      int max_landmarks, double* d_lm_center, int32_t* d_lm_label, int32_t* d_lm_count,
                      int32_t* d_lm_first, uint64_t* d_lm_sessions, double* d_lm_spread, int32_t* d_node_landmark,
                      int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_map";
    if (!no_negative(fn, {{"G", G}, {"N", N}, {"max_landmarks", max_landmarks}})) return SGPR_E_INVALID;
    if (!landmark_labels_ok(fn, h_radius, n_labels) || !radii_ok(fn, h_radius, n_labels)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_z", tau_z)) return SGPR_E_INVALID;
    if (!session_table_ok(fn.c_str(), "", h_starts, n_sessions, G)) return SGPR_E_INVALID;
    if (!lm_size_ok(G, N)) {
        set_error(fn + ": G N = " + std::to_string((long long)G * N) + " exceeds the int32 node index");
        return SGPR_E_INVALID;
    }
    if (G == 0 || N == 0) return SGPR_OK;
    const bool records = d_lm_center && d_lm_label && d_lm_count && d_lm_first && d_lm_sessions && d_lm_spread;
    if (!d_centers || !d_labels || !d_poses || (!records && max_landmarks > 0) || !d_node_landmark || !d_num || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t P = (size_t)G * (size_t)N;
    if (!workspace_ok(fn, workspace_bytes, lm_core_workspace_bytes(P))) return SGPR_E_INVALID;

    LmCoreJob job = {};
    job.centers = d_centers;
    job.labels = d_labels;
    job.poses = d_poses;
    job.G = G;
    job.N = N;
    job.h_starts = h_starts;
    job.n_sessions = n_sessions;
    job.h_radius = h_radius;
    job.n_labels = n_labels;
    job.tau_z = tau_z;
    job.max_landmarks = max_landmarks;
    job.lm_center = d_lm_center;
    job.lm_label = d_lm_label;
    job.lm_count = d_lm_count;
    job.lm_first = d_lm_first;
    job.lm_sessions = d_lm_sessions;
    job.lm_spread = d_lm_spread;
    job.node_landmark = d_node_landmark;
    job.num = d_num;
    return lm_core_launch("sgpr_landmark_map", job, d_workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"

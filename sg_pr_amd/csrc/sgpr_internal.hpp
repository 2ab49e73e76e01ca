// Internal declarations shared by the translation units of libsgpr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <atomic>
#include <string>

#include "sgpr.h"
#include "sgpr_model.hpp"

namespace sgpr {

// (shape constants, dims predicates, head_range and the host-side packer: sgpr_model.hpp)

// Device-resident, kernel-ready weights (all pointers into one allocation).
//   EdgeConv layer l (order: s_conv1, s_conv2, s_conv3, f_conv1, f_conv2, f_conv3):
//     wf[l] : [2*cout][kp] row-major.  rows [0,cout)      = s * W[:, :C]          (acts on x_j)
//                                      rows [cout,2cout)  = s * (W[:, C:] - W[:, :C])  (acts on x_i)
//     tb[l] : [cout] = beta - mean * s,  s = gamma / sqrt(var + 1e-5)   (eval BatchNorm folded)
struct DevWeights {
    const float* wf[6];             // folded fp32 weights [2*cout][kp] (a rows, then b rows); host-side source of wb
    // the same weights as three bf16 planes (w = hi + mid + lo, exact to 24 bits) in MFMA operand order:
    // [column tile][k-step][plane][lane][8]  (lane = 16*lq + l15 holds row ct*16 + l15, k = 32*step + 8*lq + 0..7;
    // first layers, K = 16: one step, k = 4*lq + 0..3 then four zeros)
    const unsigned short* wb[6];
    // ... and as two f16 planes (w = hi + lo, 22 bits), same operand order with two planes per k-step: the default
    const unsigned short* wh[6];
    const float* tb[6];
    int kp[6];
    int cout[6];
    const float* wf_end;  // [32][64] folded
    const unsigned short* wb_end;   // conv_end in the wb layout (2 column tiles, 2 k-steps)
    const unsigned short* wh_end;   // conv_end in the wh layout
    const float* tb_end;  // [32]
    const float* att_w;   // [32][32]
    const float* ntn_w;   // [32][32*16]   (weight_matrix.view(F3,-1), col = j*16 + t)
    const float* ntn_wt;  // the same tensor as [i][t][j] (ntn_prep_kernel reads 16 consecutive j per lane group)
    const float* ntn_wb;  // [16][64]
    const float* ntn_bias;  // [16]
    const float* fc1_w;   // [16][16]
    const float* fc1_b;   // [16]
    const float* fc2_w;   // [16]
    const float* fc2_b;   // [1]
    float head_scale;     // 2^k of the scoring head's f16 planes and -log2(e) 2^-k (head_range)
    float head_nl2e;
    // Semantic branch on label super-nodes, what does not depend on the graph (sgpr_embed.hip, sem_table_kernel; filled on
    // the device at sgpr_create by the instructions of the per-graph path; NULL: the per-graph path computes it).  A label
    // row of layer 1 has two versions - "fewer than K nodes carry the label" (bit 1: the padding representative is among
    // its neighbours) or not (bit 0) -, rows 12..15 (representative, unused) have one:
    const float* sem_g;   // [2][2][16][16] <x1_l (version p), x1_j (version q)> of the layer-1 rows (layer 2's Gram tile)
    const float* sem_xx;  // [2][16]        |x1_j|^2
    const float* sem_a2;  // [2][16][64]    layer 2's per-node term a = W1' x1
    const float* sem_b2;  // [2][16][64]    ... and b = (W2 - W1)' x1 + t
};

// Any-shape model (sgpr_generic.hip): the folded fp32 weights at the model's own dimensions, for what the tuned kernels
// are not built for - architectures beyond the built shape, node_num > SGPR_MAX_NODES, K > SGPR_MAX_K.
// (limits: SGPR_GENERIC_MAX_*, sgpr_model.hpp)
struct GenericModel {
    int L, f1, f2, f3, T, B, cmax;      // cmax: widest activation row (max of 3, L, f1, f2, f3)
    int cin[6], cout[6];                // EdgeConv blocks: xyz branch (s_conv1..3), then the semantic branch (f_conv1..3)
    // (the 1x1 convolutions are stored input-channel-major with the output channels padded to a multiple of 8, cout8:
    //  the 8 weights a wave needs for one input channel are contiguous and wave-uniform)
    const float* wa[6];                 // [cin][cout8]  s * W[:, :cin]            (acts on x_j)
    const float* wb[6];                 // [cin][cout8]  s * (W[:, cin:] - W[:, :cin])   (acts on x_i)
    const float* tb[6];                 // [cout]        beta - mean * s,  s = gamma / sqrt(var + 1e-5)
    const float* w_end;                 // [2 f3][f3 rounded up to 8]   conv_end, BatchNorm folded
    const float* t_end;                 // [f3]
    const float* att_w;                 // [f3][f3]
    const float* ntn_w;                 // [f3][f3][T]
    const float* ntn_wb;                // [T][2 f3]
    const float* ntn_bias;              // [T]
    const float* fc1_w;                 // [B][T]
    const float* fc1_b;                 // [B]
    const float* fc2_w;                 // [B]
    const float* fc2_b;                 // [1]
    float head_scale, head_nl2e;        // head_range of fc1_w / fc2_w (the matrix-core tail, sgpr_wide.hip)
    int head_f16;                       // ... and whether its fold fits the f16 range
};

// Matrix-core form of a GenericModel for MODERATELY larger architectures (sgpr_wide.hip): labels <= 32, filters_1 / 2 <= 128,
// filters_3 <= 64; every width padded to a multiple of 32 with zero weights (exact: a padded channel is lrelu(0 + 0) = 0
// and meets zero weights in the next layer).  Weights as two f16 planes in MFMA operand order, like DevWeights::wh.
// (limits: SGPR_WIDE_MAX_*, sgpr_model.hpp)
struct WideModel {
    int ok;                                // 0: this architecture / these weights are not served (limits, f16 range)
    int L, f3, F3P;                        // F3P = filters_3 padded
    int cinP[6], coutP[6];                 // GenericModel's layer order: xyz layers 0..2, semantic 3..5
    const unsigned short* wh[6];           // [2 coutP / 16 column tiles: a rows, then b rows][cinP / 32 k-steps][2 planes][64 lanes][8]
    const float* tbp[6];                   // [coutP]
    const unsigned short* wh_end;          // [F3P / 16][2 F3P / 32][2][64][8]: conv_end on cat(xyz3 [F3P], sem3 [F3P])
    const float* tbp_end;                  // [F3P]
    const float* att_w;                    // [f3][f3] (the GenericModel's)
};

}  // namespace sgpr

struct sgpr_handle {
    int device;
    int num_cus;
    sgpr_dims dims;
    float* d_blob;       // owns the packed weights
    size_t blob_floats;
    int32_t* d_status;   // label-error flag
    sgpr::DevWeights w;
    // debug / ablation hooks (sgpr_debug_set_*): per handle, off by default; the only mutable state of a handle
    int dbg_skip;
    unsigned long long* dbg_prof;
    int f16_weights;     // every folded weight fits the f16 range (else the wide-range layouts are used throughout)
    int head_f16;        // the scoring head's fold fits the f16 range (else the tails take the wide-range instance)
    int generic_only;    // the architecture is larger than the built shape: every call runs on the any-shape kernels
    float* d_gblob;      // owns the any-shape model's weights
    sgpr::GenericModel gm;
    void* d_wblob;       // owns the matrix-core form of the any-shape model (wm.ok != 0)
    sgpr::WideModel wm;
};

namespace sgpr {

// LDS plan of the embed kernel for one (N, k); computed on the host, passed by value.
struct EmbedPlan {
    int N;           // slots per graph in global memory (node_num)
    int NC;          // upper bound of the slots PROCESSED per graph (node_cap <= N): sizes every LDS buffer
    int NP, k, kp;   // NP = NC rounded up to 16
    int nt;          // threads per workgroup: 256 (LDS <= 80 KB: two or more workgroups per CU) or 512
    int pitchD;      // ints per row of the ranking-key chunk
    int RC;          // rows per key chunk (multiple of 16); RC == NP => symmetric Gram
    int P;           // lanes per row in the selection phase (power of two)
    int seg;         // candidates per lane (multiple of 4, <= 32)
    int kpitch;      // u16 entries per row of the neighbour list
    int pitchA;      // floats per row of the gather target A
    int overlap;     // 1: key matrix resident, selection (half the waves) overlaps the GEMMs (other half)
    int park_in_lds; // xyz3 parked in LDS (1) or in the global workspace (0)
    int park_hybrid; // park_in_lds == 0 only: the 16 super-node rows of the first branch (+ its scratch) still sit in LDS
                     // (offPark); only a graph that takes the generic semantic branch uses its rows of the global workspace
    int small_park;  // 1: the LDS park holds only the 16 super-node rows (lean production launches): a graph that needs the
                     // generic semantic branch is re-embedded by the second pass
    int alias_da;    // 1: the key matrix / chunk D shares the A region (a barrier separates selection and GEMMs)
    int lean;        // 1: NP <= 64 - one wave per 16-row tile, weight-stationary GEMMs, <= 168-VGPR kernel instance
    int big;         // owned-rows instance for plans beyond 64 rows (sgpr_embed.hip, embed_big_kernel): 0 no; 1 keys in the
                     // chunked plans' operation order, 2 in the resident plans' (what the full plan of the same launch uses)
    int xplanes;     // 1: X rows are bf16 / f16 planes; 0: fp32 rows (272 B) split when loaded
    int fmt;         // X layout: 2 = two f16 planes (272 B rows, the default), 1 = three bf16 planes (400 B), 0 = fp32 rows
    int rowb;        // bytes per X row
    int offX, offA, offD, offPark, offXX, offRed, offIdx;  // byte offsets into dynamic LDS
    int sem_wave;    // big != 0 only: the super-node branch has LDS of its own (offSem) and runs on ONE otherwise idle wave beside
    int offSem;      // the first xyz layer's selection (embed_graph); 0: on the whole workgroup, ahead of the xyz layers
    int lds_bytes;
};
bool make_embed_plan(int N, int node_cap, int k, EmbedPlan* plan, bool wide_range = false, bool small_park = false,
                     int min_nt = 0);

struct EmbedArgs {
    const float* centers;   // packed input, or
    const int32_t* labels;
    const long long* rag_off;       // ragged packed input (sgpr_embed_ragged): graph g owns nodes [rag_off[g], rag_off[g+1]) of
    const signed char* rag_lab;     // centers [S][3] / rag_lab [S]; the N - count padding slots exist only in registers
    const float* dense;     // dense [G][3+L][N] input (centers/labels NULL)
    const int32_t* ids;     // optional [G] graph indices: workgroup b embeds graph ids[b] (sgpr_embed_ordered)
    const float* dense2;    // optional second dense tensor: graphs g >= g_split read dense2[g - g_split]
    int g_split;
    int num_labels;         // label classes of the loaded checkpoint (<= kLabels): dense tensors have 3 + num_labels channels,
                            // a packed label outside [-1, num_labels) is an error (the reference raises KeyError, sg_net.py:277)
    int G;
    float* pooled;
    float* att;
    float* emb;
    float* dbg_layers;
    int32_t* dbg_knn;
    float* park_ws;         // [G][NP][32] when !park_in_lds
    unsigned char* redo;    // [launch slots] written by the f16 instance: 1 = the graph left the f16 range -> embed_redo_kernel
    unsigned* redo_count;   // one word: receives sem_epoch when any slot asks for the second pass (else untouched)
    // no promise from the caller and a plan for fewer slots than node_num (launch_embed, "auto" launches): a graph that
    // needs more processed slots than the plan holds is handed on instead of being an error - redo[slot] = 3 and the
    // launch's token in over_count (the owned-rows instance for node_num slots takes those graphs in a launch of its own),
    // or a plain second-pass request when over_count is NULL
    unsigned* over_count;
    int auto_over;          // 1: the hand-over above applies; 2 (embed_big_kernel only): persistent launch over the slots flagged 3
    int over_cap;           // slots the hand-over launch is sized for: the caller's node_cap when one above 64 was promised, else node_num
    // split launch (sgpr_embed.hip): workgroup s < G (a PRODUCER: the semantic half of launch slot s) publishes the 16
    // sem3 rows of the slot in sem_tab[s][16][32] and sem_flag[s] = token(s); workgroup G + s (the CONSUMER: the xyz half)
    // picks them up before conv_end.  Producers own the lower block indices and are therefore dispatched first - the
    // forward-progress argument of the hand-over (a waiting consumer never holds a CU its own producer still needs)
    // depends on that order.  sem_tab == NULL: the unsplit launch
    float* sem_tab;
    unsigned long long* sem_flag;
    unsigned sem_epoch;         // this launch's token: distinguishes its flags / redo_count from whatever the workspace held
    int32_t* status;
    unsigned long long* prof;   // optional [8] per-phase cycle counters (sgpr_debug_set_profile_buffer)
    int promise;                // the caller's node_cap (or N): checked even when the plan ignores it
    int skip;                   // debug/ablation only (sgpr_debug_set_profile_buffer's companion): phases to skip
};

// (sgpr_metrics.hip's matrix consumers and the fused evaluation epilogues of sgpr_score.hip label pairs alike)
// how a pair (row r of the rectangle, column c) is labelled
struct PairTruth {
    int row0;                 // global index of row 0 (rows are a shard of the square matrix)
    const double* pose;       // [>= row0 + R and >= M][2] planar pose (x, z) or NULL; float64 like the reference
    double d_pos, d_neg;      // positive if distance <= d_pos, negative if >= d_neg, ignored in between
    const signed char* gt;    // explicit labels [R][ldg]: 1 / 0 / negative = ignore (used when pose == NULL)
    int64_t ldg;
};

// 1 positive, 0 negative, -1 ignored
__device__ __forceinline__ int classify_pair(const PairTruth& t, int r, int c, double px, double pz, double lo2, double hi2) {
    if (t.pose) {
        // utils.py:36 in float64, operation by operation (no fused multiply-add)
        const double dx = px - t.pose[2 * c], dz = pz - t.pose[2 * c + 1];
        const double s2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dz, dz));
        // sqrt is monotone and correctly rounded: away from the two thresholds the squared distance decides; only
        // within a relative 1e-12 of them is the reference's `sqrt(...) <= t` evaluated literally
        if (s2 < lo2 * (1.0 - 1e-12)) return 1;
        if (s2 > lo2 * (1.0 + 1e-12) && s2 < hi2 * (1.0 - 1e-12)) return -1;
        if (s2 > hi2 * (1.0 + 1e-12)) return 0;
        const double d = sqrt(s2);
        return d <= t.d_pos ? 1 : (d >= t.d_neg ? 0 : -1);
    }
    const int g = t.gt[(int64_t)r * t.ldg + c];
    return g < 0 ? -1 : (g != 0);
}

// classify_pair's pose rule for sgpr_score_mine / sgpr_mine_rows with floating-point contraction off: __dmul_rn /
// __dadd_rn are a plain x * y and x + y here, and with HIP's default contraction the compiler fuses dz * dz into the
// sum - one rounding fewer than utils.py:36 / PairSet._targets, which flips pairs at exactly d_pos or d_neg (a pose
// (1.8, 2.4) from the origin: 9.0 unfused, 9.000000000000002 fused).  (classify_pair itself is left as it is: its
// instances' code is unchanged by this addition.)
__device__ __forceinline__ int classify_pose_exact(const double* __restrict__ pose, int c, double px, double pz,
                                                   double d_pos, double d_neg, double lo2, double hi2) {
#pragma clang fp contract(off)
    const double dx = px - pose[2 * (size_t)c], dz = pz - pose[2 * (size_t)c + 1];
    const double s2 = dx * dx + dz * dz;
    if (s2 < lo2 * (1.0 - 1e-12)) return 1;
    if (s2 > lo2 * (1.0 + 1e-12) && s2 < hi2 * (1.0 - 1e-12)) return -1;
    if (s2 > hi2 * (1.0 + 1e-12)) return 0;
    const double d = sqrt(s2);
    return d <= d_pos ? 1 : (d >= d_neg ? 0 : -1);
}

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);
// after a kernel launch: SGPR_OK, or hip_fail of what hipGetLastError() reports
int launched(const char* what);

inline size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- the argument bundles of the retrieval launchers ("Launcher bundles").  Plain host structs: a public
//      entry point fills each once, by named members or the maker beside the struct, and hands it on by const&; a
//      launcher fills its kernel's own argument struct from them.  A new retrieval launcher takes these.
struct ScoreBlock {            // a resident matrix, or one score block of a row-blocked call
    const float* score;        // [R][ld]
    int R, M;
    int64_t ld;
};

struct PooledRect {            // the pooled operands of the fused forms
    const float* rows;
    int R;
    const float* cols;
    int M;
};

struct Eligible {              // which columns a row may list (tk_bounds)
    const int32_t* row_self;   // [rows] the column of each row's own frame, or nullptr: row0 + r
    int row0, window, causal;  // window < 0: none
    // the same rule for the rows from r on: the one place that rebases row_self and row0
    Eligible from(int r) const { return {row_self ? row_self + r : nullptr, row0 + r, window, causal}; }
    // the session pipeline's selection: the filter has applied the window
    Eligible without_window() const { return {row_self, row0, -1, causal}; }
};
inline Eligible eligible(const int32_t* row_self, int row0, int window, int flags) {
    return {row_self, row0, window, (flags & SGPR_TOPK_CAUSAL) ? 1 : 0};
}

struct SeqSpec {               // the sequence match: diagonal, path set or sessions
    int ctx, L, dirs;          // dirs: SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE, at least one
    const int32_t* offsets;    // host table [n_paths][L] (already checked; copied into the launch), nullptr: the unit diagonal
    int n_paths;
    const int32_t* row_starts; // host session tables (already checked; copied into the launch), nullptr: one session
    int n_row;
    const int32_t* col_starts;
    int n_col;
    int min_terms;             // 1..L (the session range selection)
    SeqSpec paths(const int32_t* off, int n) const {
        SeqSpec s = *this;
        s.offsets = off;
        s.n_paths = n;
        return s;
    }
    SeqSpec sessions(const int32_t* rows, int nr, const int32_t* cols, int nc) const {
        SeqSpec s = *this;
        s.row_starts = rows;
        s.n_row = nr;
        s.col_starts = cols;
        s.n_col = nc;
        return s;
    }
};
inline SeqSpec seq_spec(int ctx, int L, int flags, int min_terms = 1) {   // the unit diagonal in one session
    SeqSpec s = {};
    s.ctx = ctx;
    s.L = L;
    s.dirs = flags & (SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE);
    s.min_terms = min_terms;
    return s;
}

struct RangeOut {              // where a range selection's result goes
    int32_t* rows;
    int32_t* cols;
    float* vals;
    unsigned char* codes;      // directions / codes of the sequence forms, or nullptr
    int64_t cap;
    int64_t* row_ptr;          // [output rows + 1] of this launch's first output row
    int rout0;                 // output row of that row
    unsigned long long* count;
    int accumulate;            // positions continue from *count
    void* ws;
    int32_t* status;
    // the launch whose first output row is the call's row o, with its workspace
    RangeOut at(int o, void* w) const {
        RangeOut r = *this;
        r.row_ptr = row_ptr + o;
        r.rout0 = o;
        r.accumulate = o > 0;
        r.ws = w;
        return r;
    }
};
// a call's output before any launch: row 0, nothing accumulated, no workspace yet
inline RangeOut range_out(int32_t* rows, int32_t* cols, float* vals, unsigned char* codes, int64_t cap, int64_t* row_ptr,
                          unsigned long long* count, int32_t* status) {
    RangeOut r = {};
    r.rows = rows;
    r.cols = cols;
    r.vals = vals;
    r.codes = codes;
    r.cap = cap;
    r.row_ptr = row_ptr;
    r.count = count;
    r.status = status;
    return r;
}

struct ListOut {               // k-entry lists per row
    float* val;                // [rows][k]
    int32_t* idx;
    int k;
    unsigned char* codes;      // [rows][k] directions / codes of the ranking pipeline (launch_seq_dirs), or nullptr
    ListOut at(size_t row) const { return {val + row * k, idx + row * k, k, codes ? codes + row * k : nullptr}; }
};

struct MineSpec {              // the pose-class condition of mined pairs
    int positives;             // SGPR_MINE_POSITIVES, else the negatives
    const double* col_pose;
    const double* row_pose;    // [rows][2] or nullptr: the pose of the row's own column
    double d_pos, d_neg;
    MineSpec from(int r) const {
        MineSpec m = *this;
        if (m.row_pose) m.row_pose += 2 * (size_t)r;
        return m;
    }
};
inline MineSpec mine_spec(int flags, const double* col_pose, const double* row_pose, double d_pos, double d_neg) {
    MineSpec m;
    m.positives = (flags & SGPR_MINE_POSITIVES) ? 1 : 0;
    m.col_pose = col_pose;
    m.row_pose = row_pose;
    m.d_pos = d_pos;
    m.d_neg = d_neg;
    return m;
}

struct FilterOut {             // a filter's Q block and the direction / code taken
    float* out;                // [rows][ldo]
    int64_t ldo;
    unsigned char* code;       // [rows][ldc] or nullptr
    int64_t ldc;
};

int launch_embed(const sgpr_handle* h, const EmbedPlan& plan, const EmbedArgs& a, hipStream_t stream);
// fills table[kSemTableFloats] (layout: sem_g | sem_xx | sem_a2 | sem_b2) and *vmax_out (largest |layer-1 output|)
int launch_sem_tables(const DevWeights& w, float* d_table, float* d_vmax, hipStream_t stream);
int launch_score_pairs(const sgpr_handle* h, const float* p1, const int32_t* i1, const float* p2, const int32_t* i2,
                       int64_t P, float* score, hipStream_t stream);
size_t score_all_pairs_ws_bytes(int R, int M);
// crng: the f16 range of a larger call this rectangle is a row block of (launch_call_range), read instead of its own
int launch_score_all_pairs(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, float* score,
                           int64_t ld, void* ws, hipStream_t stream, bool wide = false, const float* crng = nullptr);
// the f16-range question of R rows scored in blocks of rb, answered once into the float4 g (ws: score_all_pairs_ws_bytes(rb, M))
int launch_call_range(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, int rb, void* ws,
                      float* g, hipStream_t stream);
size_t score_all_pairs_multi_ws_bytes(int n, const sgpr_pairs_job* jobs);
int launch_score_all_pairs_multi(const sgpr_handle* h, int n, const sgpr_pairs_job* jobs, void* ws, hipStream_t stream);
size_t score_topk_ws_bytes(const sgpr_handle* h, int R, int M, int k);
int launch_score_topk(const sgpr_handle* h, const PooledRect& p, const Eligible& e, const ListOut& out, void* ws,
                      hipStream_t stream);
// sgpr_topk_rows' selection with a row_self table, the causal rule and an output row stride of k (sgpr_metrics.hip)
int launch_topk_rows_ext(const ScoreBlock& b, const Eligible& e, const ListOut& out, int32_t* status, hipStream_t stream);
// the large-k selection of a resident n x M block into [n][k] (sgpr_select.hip); ws_clean: ws is what an earlier call on
// the same stream left (its histograms are clear)
size_t select_ws_bytes(int n, int M);
// ws_clean holds only for a block whose select_group_rows is at most that of the call before it on the same ws: a call
// leaves its own histogram rows clear and its state / counts right behind them
int select_group_rows(int n);
int launch_select_rows(const ScoreBlock& b, const Eligible& e, const ListOut& out, void* ws, bool ws_clean,
                       int32_t* status, hipStream_t stream);
// the diagonal score filter of a resident R x M matrix (sgpr_seq.hip): Q for rows ctx .. R-1 into out [R - ctx][ldo],
// the direction taken into code [R - ctx][ldc] (or nullptr); of `seq`: ctx, L, dirs
int launch_seq_filter(const ScoreBlock& b, const SeqSpec& seq, const FilterOut& out, hipStream_t stream);
// out [n][k] = dir [n][ld] at the selected columns idx [n][k] (dir == nullptr: `fixed`); 0 where idx is -1
int launch_seq_dirs(const int32_t* idx, int n, int k, const unsigned char* dir, int64_t ld, int fixed,
                    unsigned char* out, hipStream_t stream);
// the path-set score filter of a resident R x M matrix (seq_path_kernel, sgpr_seq.hip): launch_seq_filter's arguments with
// seq's path table and the winner's code (direction bit | path << 1) into out.code
int launch_seq_path_filter(const ScoreBlock& b, const SeqSpec& seq, const FilterOut& out, hipStream_t stream);
// the session-aware path-set filter of a resident R x M matrix (session_kernel, sgpr_seq.hip): launch_seq_path_filter's
// arguments (seq.offsets == nullptr: the unit diagonal) with seq's session tables and the session window on the end point
// (e.row_self [R] / e.row0 belong to the matrix's row 0; e.causal is not the filter's)
int launch_session_filter(const ScoreBlock& b, const SeqSpec& seq, const Eligible& e, const FilterOut& out,
                          hipStream_t stream);
// the peak filter of a resident n x M block (sgpr_peak.hip): out [n][ldo] = score at a peak within `radius` columns, -inf
// elsewhere; eligibility as launch_select_rows (e.row_self [n] / e.row0 belong to the block's row 0)
int launch_peak_filter(const ScoreBlock& b, const Eligible& e, int radius, float* out, int64_t ldo, hipStream_t stream);
// sgpr_score_mine on the production handle (positives: SGPR_MINE_POSITIVES, else the negatives) and its selection on a
// resident block (sgpr_mine_rows, the chunked path of the other handles; sgpr_metrics.hip)
size_t score_mine_ws_bytes(const sgpr_handle* h, int R, int M, int k);
int launch_score_mine(const sgpr_handle* h, const PooledRect& p, const Eligible& e, const MineSpec& mine,
                      const ListOut& out, void* ws, hipStream_t stream);
int launch_mine_rows(const ScoreBlock& b, const Eligible& e, const MineSpec& mine, const ListOut& out, int32_t* status,
                     hipStream_t stream);
size_t score_above_ws_bytes(const sgpr_handle* h, int R, int M);
size_t rows_above_ws_bytes(int R);
int launch_above_empty(int R, int64_t* row_ptr, unsigned long long* count, hipStream_t stream);
// (out.row_ptr == nullptr: the front of out.ws holds it; out.status is not read: the handle's)
int launch_score_above(const sgpr_handle* h, const PooledRect& p, const Eligible& e, float thr, const RangeOut& out,
                       hipStream_t stream);
// the range selection of a resident R x M block (sgpr_rows_above, the chunked path of sgpr_score_above): out.row_ptr
// [R + 1] of the block's rows, output rows out.rout0 + r
int launch_rows_above(const ScoreBlock& b, const Eligible& e, float thr, const RangeOut& out, hipStream_t stream);
// above_scan_kernel on its own: cnt [n] -> row_ptr [n + 1] and *count, both continuing from *count with accumulate
int launch_above_scan(const int32_t* cnt, int n, int64_t* row_ptr, unsigned long long* count, int accumulate,
                      hipStream_t stream);
// the range selection of the sequence-matched score of a resident R x M block (sgpr_seq.hip; sgpr_seq_rows_above and
// each row block of sgpr_score_seq_above): the eligible pairs of rows ctx .. R-1 with Q >= thr, row-major, as output
// rows out.rout0 + r - ctx; e.row_self [R] / e.row0 belong to the block's row 0, out.row_ptr [R - ctx + 1] to its first
// output row.  out.ws: seq_above_ws_bytes(R - ctx, M)
size_t seq_above_ws_bytes(int n, int M);
int launch_seq_above(const ScoreBlock& b, const SeqSpec& seq, const Eligible& e, float thr, const RangeOut& out,
                     hipStream_t stream);
// seq_above_rowscan_kernel on its own (sgpr_seq.hip): seg [n][nseg] -> exclusive offsets in place, cnt [n] = row totals
int launch_seq_above_rowscan(int32_t* seg, int n, int nseg, int32_t* cnt, hipStream_t stream);
// launch_seq_above on the session-aware path-set score with a minimum term count (session_above_kernel, sgpr_seq.hip; sgpr_session_rows_above
// and each row block of sgpr_score_session_above): launch_session_filter's paths, tables and session window, codes in
// place of directions.  out.ws: seq_above_ws_bytes(R - ctx, M)
int launch_session_above(const ScoreBlock& b, const SeqSpec& seq, const Eligible& e, float thr, const RangeOut& out,
                         hipStream_t stream);
// the fused evaluation epilogues of the all-pairs tail (production handle): T >= 0 the threshold counts (count == NULL,
// d_out [T + 3]), T < 0 the positives (out [cap], count [2])
size_t score_eval_ws_bytes(const sgpr_handle* h, int R, int M, int T);
int launch_score_eval(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, const PairTruth& truth,
                      float* out, int64_t cap, unsigned long long* count, const float* thr, int T,
                      const sgpr_rank_group* rank, int gpt, const unsigned long long* at_least, unsigned long long* d_out,
                      void* ws, hipStream_t stream);
// sgpr_pair_positives' kernel without clearing d_count: the appends of a row block continue the list (sgpr_metrics.hip)
int launch_pair_positives_more(const sgpr_handle* h, const float* score, int R, int M, int64_t ld, const PairTruth& truth,
                               float* out, int64_t cap, unsigned long long* count, hipStream_t stream);
// ... and sgpr_pair_threshold_counts' two kernels without its argument checks; accumulate: d_out [T + 3] keeps what the
// row blocks before this one left in it.  slabs: sgpr_pair_threshold_counts_workspace_bytes(h, T)
int launch_pair_counts_more(const sgpr_handle* h, const float* score, int R, int M, int64_t ld, const PairTruth& truth,
                            const float* thr, int T, const sgpr_rank_group* rank, int gpt,
                            const unsigned long long* at_least, unsigned long long* d_out, unsigned* slabs,
                            int accumulate, hipStream_t stream);
size_t score_pair_list_ws_bytes(int NR, int M);
int launch_score_pair_list(const sgpr_handle* h, const float* rows, const float* cols, int M, const int32_t* plan,
                           int NR, int NI, int64_t P, float* score, void* ws, hipStream_t stream, bool exact = false);
int generic_embed_slots(const sgpr_handle* h, int G);
size_t generic_embed_ws_bytes(const sgpr_handle* h, int G, int N, int k);   // 0: the working memory fits LDS
size_t generic_embed_lds_bytes(const sgpr_handle* h, int N, int k);
int launch_embed_generic(const sgpr_handle* h, const EmbedArgs& a, int N, int k, void* ws, hipStream_t stream);
// the matrix-core any-shape embed: does this handle / launch take it, its LDS, the launch (flags the graphs whose values
// leave the f16 range in a.redo - the plain-fp32 kernel then embeds those, launch_embed_generic with a.auto_over == 7)
bool wide_embed_serves(const sgpr_handle* h, const EmbedArgs& a, int N, int k);
size_t wide_embed_lds_bytes(int N);
int launch_embed_wide(const sgpr_handle* h, const EmbedArgs& a, int N, int k, hipStream_t stream);
// ... and its dense all-pairs tail (pooled width <= 64, tensor / bottleneck neurons <= 32): *d_gate = the device word the
// plain-fp32 kernel behind the call tests (non-zero: inputs outside the f16 range, the rectangle is its)
bool wide_tail_serves(const sgpr_handle* h);
size_t wide_tail_ws_bytes(int R, int M);
// fresh = false: the header in ws is not cleared - it already holds the range maxima of the caller's whole rectangle,
// accumulated by launch_wide_tail_prep over each of its row blocks after one clear (a row-blocked call's range is the call's)
int launch_score_all_pairs_wide_any(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, float* score,
                                    int64_t ld, void* ws, const unsigned** d_gate, hipStream_t stream, bool fresh = true);
int launch_wide_tail_prep(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, void* ws,
                          hipStream_t stream);
// list form (M == 0: pair p = (i1 ? i1[p] : p, i2 ? i2[p] : p) -> score[p]) or dense rectangle (M > 0: P = R * M pairs -> score[r * ld + c])
int launch_knn_any(const float* x, int B, int C, int N, int k, int64_t* idx, hipStream_t stream);
int launch_attention_any(const float* w, const float* emb, int B, int N, int F, float* rep, float* att, hipStream_t stream);
int launch_ntn_any(const float* w, const float* wb, const float* bias, const float* e1, const float* e2, int64_t P, int F,
                   int T, float* out, hipStream_t stream);
int launch_score_generic(const sgpr_handle* h, const float* p1, const int32_t* i1, const float* p2, const int32_t* i2,
                         int64_t P, int M, float* score, int64_t ld, hipStream_t stream, const unsigned* d_gate = nullptr);
int launch_score_plan_generic(const sgpr_handle* h, const float* rows, const float* cols, const int32_t* plan, int NR, int NI,
                              int64_t P, float* score, hipStream_t stream);
int launch_ntn(const float* w, const float* wb, const float* bias, const float* e1, const float* e2, int64_t B,
               float* out, hipStream_t stream);
int launch_knn(const float* x, int B, int C, int N, int k, int64_t* idx, hipStream_t stream);
int launch_graph_feature(const float* x, const int64_t* idx, int B, int C, int N, int k, float* out, hipStream_t stream);
int launch_attention_pool(const float* w, const float* emb, int B, int N, float* rep, float* att, hipStream_t stream);

// geometric verification of P candidate pairs, one workgroup each (sgpr_verify.hip); arguments already checked
int launch_verify_pairs(const float* ca, const int32_t* la, int GA, const float* cb, const int32_t* lb, int GB, int N,
                        const int32_t* ia, const int32_t* ib, int64_t P, float tau_edge, float tau_in, float tau_z,
                        float min_base, int max_hyp, sgpr_verify_result* out, hipStream_t stream);

// pairwise consistency of C closures and the greedy clique of every group (sgpr_consistency.hip); arguments already checked
size_t closure_consistency_ws_bytes(int C);
size_t consistent_set_ws_bytes(int C);
int launch_closure_consistency(const int32_t* rows, const int32_t* cols, const double* T, int C, const double* Xr, int MR,
                               const double* Xc, int MC, const int32_t* group, int n_groups, double max_trans,
                               double min_cos, double lever_gain, unsigned long long* adj, int32_t* degree, void* ws,
                               hipStream_t stream);
int launch_consistent_set(const unsigned long long* adj, int C, const int32_t* group, int n_groups, int32_t* rank,
                          int32_t* group_size, void* ws, hipStream_t stream);

size_t size_order_ws_bytes(int G);
int launch_size_order(const float* centers, const int32_t* labels, const long long* rag_off, int G, int N, int k,
                      int num_labels, int32_t* order, int32_t* info, void* ws, hipStream_t stream);

size_t cluster_ws_bytes(int P);
int launch_cluster_scan(const float* pts, int stride, const uint32_t* label, int P, int max_nodes, double* centers,
                        int32_t* node_labels, int32_t* node_sizes, int32_t* point_node, int32_t* num_nodes, void* ws,
                        hipStream_t stream);

int launch_graph_edges(const float* pts, int stride, const int32_t* point_node, int P, int n, const double* centers,
                       double* min_dis, void* ws, hipStream_t stream);

// eligibility of column c for a row whose own frame is s: c < M and (c < ea or c > eb) - the window [s - w, s + w] and,
// causal, everything from s on are cut out
__device__ __forceinline__ void tk_bounds(long long s, int window, int causal, int& ea, int& eb) {
    const long long w = window < 0 ? 0 : window;
    long long a = window < 0 ? (causal ? s : 0x7fffffffLL) : s - w;
    long long b = (causal || window < 0) ? 0x7fffffffLL : s + w;
    ea = (int)(a < -1 ? -1 : (a > 0x7fffffffLL ? 0x7fffffffLL : a));
    eb = (int)(b < -2 ? -2 : (b > 0x7fffffffLL ? 0x7fffffffLL : b));
}

// The ReLU of the exact fp32 tails (per-pair scoring, the f16 tails' fallback, the any-shape tail, training): fmaxf(NaN, 0)
// is 0, which would score a graph whose pooled vector is NaN - the library's own error marker - like a healthy one.
// A NaN stays a NaN; every other value gets fmaxf's bits.
__device__ __forceinline__ float relu_keep_nan(float x) { return x != x ? x : fmaxf(x, 0.f); }

// sgpr_knn's ranking, shared by its two instances (knn_kernel, generic_knn_kernel) so that they return the same lists:
//   key(i, j) = |x_i|^2 - (2 x_i.x_j - |x_j|^2) = -pd[i][j],  |x|^2 = rounded squares summed in channel order,
//   x_i.x_j = an fma chain in channel order from the rounded first product (no contraction beyond the fmaf calls)
__device__ __forceinline__ float knn_sq_norm(const float* v, int C, size_t stride) {
    float s = __fmul_rn(v[0], v[0]);
    for (int c = 1; c < C; ++c) s = __fadd_rn(s, __fmul_rn(v[(size_t)c * stride], v[(size_t)c * stride]));
    return s;
}
__device__ __forceinline__ float knn_key(float xi2, float xj2, float dot) { return __fsub_rn(xi2, fmaf(2.f, dot, -xj2)); }
// (key, index) under one total order: the order-preserving image of the key (-0 as +0, +inf after every finite key, NaN
// after everything) above the candidate index - the smaller value ranks first, equal keys lower index first
__device__ __forceinline__ unsigned long long knn_rank(float key, int j) {
    unsigned img = 0xffffffffu;
    if (key == key) {
        key += 0.0f;
        const unsigned u = __float_as_uint(key);
        img = u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
    }
    return ((unsigned long long)img << 32) | (unsigned)j;
}

// Raising a kernel's dynamic-LDS limit (hipFuncSetAttribute) applies to the CURRENT device only: remembered per device
// (one bit each; a process that drives several GPUs raises it once on each), with a message that says what did not fit -
// a part with 64 KB of LDS per workgroup cannot run the kernels that stage a whole graph / histogram in 130 - 160 KB.
struct LdsLimitOnce {
    std::atomic<unsigned long long> done{0ull};   // (threads that drive different GPUs share it; setting the attribute twice is idempotent)
};
int raise_lds_limit(LdsLimitOnce* once, const void* kernel, int bytes, const char* what);

// makes `device` current for the lifetime of the object and restores the caller's device afterwards
struct DeviceGuard {
    int prev;
    bool switched;
    explicit DeviceGuard(int device) : prev(-1), switched(false) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

}  // namespace sgpr

/*
 * sgpr.h - C ABI of the MI355X-native SG_PR pair-scoring engine (libsgpr_hip.so).
 *
 * The reference (kxhit/SG_PR) is pure Python/PyTorch and has no FFI layer; its
 * boundary for the hot path is the Python API of `sg_net.SG` plus the
 * `model.pth` state-dict layout.  This header is the C-ABI a
 * maintainer binds *below* that API: plain pointers and sizes, no torch types.
 * Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - every `d_` pointer is DEVICE memory owned by the caller (fp32 / int32,
 *     dense row-major); `stream` is a hipStream_t passed as void* (NULL = the
 *     null stream).  Launches are asynchronous on that stream.
 *   - the engine owns only its packed-weights copy inside the handle; no
 *     allocation happens inside launch calls (workspaces are passed in).
 *   - return value 0 = SGPR_OK, negative = error; sgpr_last_error() gives the
 *     message of the last failing call on the calling thread.
 *   - a handle is immutable after create => safe to use from several
 *     streams/threads (the sgpr_debug_* hooks are the one exception: they are
 *     per handle, off by default and not meant for production).  One process
 *     per GPU.
 *   - the device status word (label / node_cap / row_self reports) belongs to
 *     the handle, not to a call: sgpr_check_status reports and clears the
 *     flags raised by ANY call on the handle since the last check, on any
 *     stream or thread.
 *   - results depend on the arguments alone: every workspace region is set by
 *     the call that reads it (a memset, a producer kernel or a per-call token),
 *     so a workspace may hold anything - another entry point's leftovers
 *     included - and output buffers need no clearing.
 *   - every entry point that takes a handle runs on the handle's device and
 *     restores the caller's current device before it returns; the handle-free
 *     entry points (sgpr_knn, sgpr_graph_feature, sgpr_attention_pool,
 *     sgpr_ntn, sgpr_verify_pairs, sgpr_closure_consistency, sgpr_consistent_set) run on the caller's current device.
 */
#ifndef SGPR_H
#define SGPR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_ABI_VERSION 11

enum {
    SGPR_OK = 0,
    SGPR_E_INVALID = -1,   /* NULL pointer / negative count                                   */
    SGPR_E_DIMS = -2,      /* architecture beyond the any-shape limits, or an entry point the tuned kernels alone serve */
    SGPR_E_NODES = -3,     /* node_num outside [k, SGPR_ANY_MAX_NODES], or a graph exceeded node_cap  */
    SGPR_E_K = -4,         /* K outside [1, SGPR_ANY_MAX_K] or K > node_num                    */
    SGPR_E_LABEL = -5,     /* a label outside [-1, num_labels) was seen (sgpr_check_status)    */
    SGPR_E_HIP = -6,       /* HIP runtime error (message has hipGetErrorString)                */
    SGPR_E_WORKSPACE = -7, /* workspace missing or too small                                   */
    SGPR_E_BLOB = -8       /* weights blob has the wrong number of floats                      */
};

/* the tuned kernels (matrix cores, one workgroup stages a whole graph in LDS): every shipped checkpoint and config */
#define SGPR_MAX_NODES 256
#define SGPR_MAX_K 32
/* the any-shape kernels (plain fp32, activations in a global scratch area): what the reference can be configured to
 * beyond that (parser_sg.py:12-22 takes any filters_* / tensor_neurons / bottle_neck_neurons / node_num / K) */
#define SGPR_ANY_MAX_LABELS 64
#define SGPR_ANY_MAX_FILTERS 256  /* filters_1, filters_2 */
#define SGPR_ANY_MAX_FILTERS_3 128
#define SGPR_ANY_MAX_NEURONS 64   /* tensor_neurons, bottle_neck_neurons */
#define SGPR_ANY_MAX_NODES 1024
#define SGPR_ANY_MAX_K 64

typedef struct sgpr_handle sgpr_handle;

/* Architecture hyper-parameters = the `arch:` block of the reference's
 * config.yml (parser_sg.py:12-18) + number_of_labels (sg_net.py:201-203).
 * The HIP kernels are written for the architecture of every shipped
 * checkpoint, {12, 64, 64, 32, 16, 16}, and serve every architecture that is
 * no larger in any of the six: sgpr_create embeds its tensors into the built
 * shapes with zero weights for the channels it does not have, which is exact
 * (device buffers keep the built widths: pooled [G, 32], emb [G, N, 32], the
 * missing channels are 0; dense features are [G, 3 + num_labels, N]).
 * A LARGER architecture (any of the six, up to the SGPR_ANY_MAX_* limits) gets
 * an "any-shape" handle: the same entry points on plain-fp32 kernels
 * (sgpr_generic.hip) - correct against the same oracle, not tuned; the embed of
 * a model with <= 32 labels and filters <= 128 / 128 / 64 runs on the matrix
 * cores for node_num <= 112, K = 10, and so does sgpr_score_all_pairs(_multi)
 * when filters_3 <= 64 and tensor / bottleneck neurons <= 32 and the caller
 * passes the workspace the _workspace_bytes call asks for (sgpr_wide.hip;
 * without a workspace: the plain-fp32 kernel) - with device
 * buffers of the model's own width (pooled [G, filters_3], emb [G, N, filters_3]:
 * sgpr_pooled_width).  Not served on such a handle: sgpr_embed_debug's dumps
 * (-> SGPR_E_DIMS; sgpr_score_pair_list walks its plan pair by pair there: the
 * bits of sgpr_score_pairs, no workspace).  Beyond the
 * SGPR_ANY_MAX_* limits -> SGPR_E_DIMS at sgpr_create.
 * node_num in (SGPR_MAX_NODES, SGPR_ANY_MAX_NODES] or K in (SGPR_MAX_K,
 * SGPR_ANY_MAX_K] run on the any-shape embed kernel on every handle (the pooled
 * width stays the handle's). */
typedef struct sgpr_dims {
    int32_t num_labels;
    int32_t filters_1;
    int32_t filters_2;
    int32_t filters_3;
    int32_t tensor_neurons;
    int32_t bottle_neck_neurons;
} sgpr_dims;

/* Number of floats sgpr_create expects in `weights` for `dims`.
 * Blob layout = the fp32 tensors of the reference state dict
 * (sg_net.py:45-76; SURVEY.md row a-ckpt), each flattened row-major, in this order:
 *   for blk in [dgcnn_s_conv1, dgcnn_f_conv1, dgcnn_s_conv2, dgcnn_f_conv2,
 *               dgcnn_s_conv3, dgcnn_f_conv3, dgcnn_conv_end]:
 *       blk.0.weight [Cout, Cin2], blk.1.weight (gamma), blk.1.bias (beta),
 *       blk.1.running_mean, blk.1.running_var            (each [Cout])
 *   attention.weight_matrix [F3,F3]
 *   tensor_network.weight_matrix [F3,F3,T], .weight_matrix_block [T,2*F3], .bias [T]
 *   fully_connected_first.weight [B,T], .bias [B]
 *   scoring_layer.weight [1,B], .bias [1]
 * (the seven int64 num_batches_tracked scalars are not part of the blob). */
size_t sgpr_weights_count(const sgpr_dims* dims);

/* Replaces SGTrainer.setup_model's load_state_dict + .cuda() (sg_net.py:158-176):
 * folds eval-mode BatchNorm into the 1x1 convs, re-lays the weights out for the
 * kernels and uploads them to `device`.  `weights` is HOST memory. */
int sgpr_create(const float* weights, size_t n_floats, const sgpr_dims* dims, int device, sgpr_handle** out);
void sgpr_destroy(sgpr_handle* h);

/* Floats per row of the handle's pooled / emb buffers: 32 (the built width) for every architecture the tuned kernels
 * serve, filters_3 on an any-shape handle.  sgpr_is_any_shape: 1 for a handle of a larger architecture. */
int sgpr_pooled_width(const sgpr_handle* h);
int sgpr_is_any_shape(const sgpr_handle* h);

/* Bytes of device workspace sgpr_embed* needs for (G graphs, N slots): one flag byte per launch slot (written by the
 * f16-plane kernel instance, read by its wide-range / generic-branch second pass in the same call) plus, for N > 128,
 * the parked output of the first EdgeConv branch.  Never 0: always pass the workspace. */
size_t sgpr_embed_workspace_bytes(const sgpr_handle* h, int G, int N, int k);

/* Per-graph half of SG.forward: SG.dgcnn_conv_pass (sg_net.py:79-110 ->
 * dgcnn.knn / get_graph_feature dgcnn.py:14-49, the six EdgeConv blocks
 * sg_net.py:50-73, conv_end sg_net.py:74-76) + AttentionModule.forward
 * (layers_batch.py:28-39), fused in one kernel, one workgroup per graph.
 *   d_centers [G,N,3] f32 (0 for padded slots), d_labels [G,N] i32 (-1 = pad)
 *     = the packed form of transfer_to_torch's output (sg_net.py:250-299)
 *   d_pooled [G,F3] (required); d_att [G,N] and d_emb [G,N,F3] may be NULL. */
int sgpr_embed(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int k,
               float* d_pooled, float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes,
               void* stream);
/* Without a node_cap promise (this call; node_cap 0 below) a launch of more graphs than the device has CUs still runs on
 * the 64-row layout (K <= 16): a graph that needs more processed slots is embedded in the same call by the kernel
 * instance sized for N (same bits; no error) - data whose graphs mostly exceed 64 processed slots is served faster
 * with its node_cap (sgpr_size_order), which sizes one launch for all of them. */

/* sgpr_embed with a promise about the input: no graph of the batch needs more than `node_cap` PROCESSED slots
 * (= slots before the trailing run of m identical padding slots, + 1 when m >= k, + m otherwise; 0 = no promise).
 * The kernel sizes its LDS for node_cap instead of N: caps <= 64 (<= 48) select a fixed 64-row (48-row) layout that
 * runs four (five) workgroups per CU; caps of 65 .. 96 (K <= 16, more graphs than CUs) keep the graphs of up to 64 slots
 * on that layout and run only the others on the instance sized for node_cap; beyond, one launch sized for node_cap.  A graph that breaks the promise gets a NaN pooled vector and
 * sgpr_check_status returns SGPR_E_NODES.  Results are otherwise identical to sgpr_embed.
 * On the any-shape kernels (an architecture beyond the built shape, N > SGPR_MAX_NODES, K > SGPR_MAX_K) node_cap is
 * advisory: they size nothing by it and do not check it. */
int sgpr_embed_capped(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int node_cap,
                      int k, float* d_pooled, float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes,
                      void* stream);

/* sgpr_embed_capped over an explicit launch order: workgroup b embeds graph d_order[b] (device i32 [n_order],
 * distinct indices in [0, G), n_order <= G).  A packed graph store lists its graphs largest-first (longest
 * workgroups start first, the last round of the launch is filled by the smallest graphs - KITTI-00: -7 %), or lists
 * only the graphs that changed.  Outputs are indexed by graph id exactly as in sgpr_embed and are bit-identical to
 * it; a graph listed nowhere is not embedded and its output rows are left untouched. */
int sgpr_embed_ordered(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int node_cap,
                       int k, const int32_t* d_order, int n_order, float* d_pooled, float* d_att, float* d_emb,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* The data-set properties sgpr_embed_capped / _ordered / _ragged take, computed on the device (two small launches, no
 * host pass): d_order [G] i32 = graph indices by PROCESSED slots, largest first, stable; d_info [2] i32 = { node_cap =
 * the largest processed-slot count of the batch, graphs beyond 64 processed slots }.  Padded arrays (d_centers, d_labels;
 * d_offsets NULL) or a ragged store (d_offsets [G+1] i64; d_centers / d_labels unused, may be NULL).  The caller reads
 * d_info[0] back once per data set (4 bytes) and passes it as node_cap.  The reference has no counterpart: it pads
 * every graph to node_num (sg_net.py:258-272) and pays for node_num slots.  Workspace: sgpr_size_order_workspace_bytes(G). */
size_t sgpr_size_order_workspace_bytes(int G);
int sgpr_size_order(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, const int64_t* d_offsets, int G,
                    int N, int k, int32_t* d_order, int32_t* d_info, void* d_workspace, size_t workspace_bytes,
                    void* stream);

/* sgpr_embed_ordered over a RAGGED graph store: only the real nodes of a graph are in memory -
 *   d_centers [S,3] f32, d_labels [S] i8 (0 .. num_labels-1), d_offsets [G+1] i64: graph g owns nodes
 *   [d_offsets[g], d_offsets[g+1]) -
 * and the zero padding up to N = node_num slots that transfer_to_torch appends (sg_net.py:258-272) is made in
 * registers by the kernel.  13 bytes per real node instead of 16 per slot (KITTI-like graphs: 2.8x fewer bytes to hold
 * and to move across PCIe); results are bit-identical to sgpr_embed on the padded arrays.  d_order may be NULL
 * (n_order ignored: all G graphs in index order).  A graph with more than N nodes gets a NaN pooled vector and
 * sgpr_check_status returns SGPR_E_NODES.  Outputs (d_att [G,N], d_emb [G,N,F3]) keep the padded shape. */
int sgpr_embed_ragged(const sgpr_handle* h, const float* d_centers, const int8_t* d_labels, const int64_t* d_offsets,
                      int G, int N, int node_cap, int k, const int32_t* d_order, int n_order, float* d_pooled,
                      float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes, void* stream);

/* Same as sgpr_embed, taking the reference's dense tensor `features` [G, 3+L, N] f32
 * (data["features_1"], sg_net.py:119) - the sem block may hold any values. */
int sgpr_embed_dense(const sgpr_handle* h, const float* d_features, int G, int N, int k, float* d_pooled,
                     float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes, void* stream);

/* sgpr_embed + dumps of every intermediate for parity tests:
 *   d_layers [G,6,N,64] f32  outputs of s_conv1..3, f_conv1..3 after max-k (channels >= Cout are 0)
 *   d_knn    [G,6,N,k]  i32  neighbour lists chosen at the input of those six layers (unordered sets). */
int sgpr_embed_debug(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int k,
                     float* d_pooled, float* d_att, float* d_emb, float* d_layers, int32_t* d_knn,
                     void* d_workspace, size_t workspace_bytes, void* stream);

/* Pair-coupled half of SG.forward: TenorNetworkModule.forward
 * (layers_batch.py:70-83) + fully_connected_first/ReLU + scoring_layer/sigmoid
 * (sg_net.py:131-136) for P pairs.  Pair p scores
 *   (d_pooled1[idx1 ? idx1[p] : p], d_pooled2[idx2 ? idx2[p] : p]); idx may be NULL.
 * Non-finite pooled vectors (every scoring entry point below follows this rule): a NaN anywhere in a graph's vector - the
 * embed entry points' marker of a graph that broke its node promise - gives a NaN score for every pair of that graph,
 * never the score of a healthy graph; a +-inf gives NaN or the score of the limit, depending on the order in which the
 * kernel at work meets infinite terms; pairs of two finite graphs are not affected. */
int sgpr_score_pairs(const sgpr_handle* h, const float* d_pooled1, const int32_t* d_idx1,
                     const float* d_pooled2, const int32_t* d_idx2, int64_t P, float* d_score, void* stream);

/* The same tail for a pair LIST grouped by row graph - the shape of the reference's own evaluation loop
 * (eval_batch.py:30-36 walks `<seq>.txt`, utils.py:61-70: 10^4 - 10^5 listed pairs over 10^3 graphs, ~15 per row graph).
 * sgpr_score_pairs spends a whole wave and a 64 KB weight read on every pair; here the bilinear form is hoisted per
 * DISTINCT row graph and the listed columns of a row go through the matrix cores 16 at a time, exactly like a row of
 * the dense rectangle: on an f16 handle the scores are bit-identical to sgpr_score_all_pairs' entries at the listed
 * (row, column).  A handle whose tail runs at fp32's range (weights or scoring head outside the f16 range, debug bit 13)
 * scores the list with the kernel's exact fp32 per-pair arithmetic - sgpr_score_pairs' values to rounding, not the bits
 * of its three-plane matrix.
 *
 * sgpr_pair_plan (HOST memory in and out, no GPU work): groups pair p = (idx1[p], idx2[p]), 0 <= idx1 < R, 0 <= idx2 < M,
 * P < 2^31, by row graph (stable: a row's pairs keep their list order) and cuts every row's pairs into work items of
 * <= 16.  h_plan receives int32 words
 *     row_ids [n_rows] | item_row [n_items] | item_begin [n_items + 1] | cols [P] | pos [P]
 * (distinct row graphs ascending; per item its row as an index into row_ids and its first pair in cols / pos; per pair
 * its column graph and its position in the caller's list).  sgpr_pair_plan_ints(P, R) bounds the words needed;
 * *plan_ints returns the words written.  An index out of range -> SGPR_E_INVALID.  Build it once per list (like a launch
 * order), copy it to the device, reuse it for every call.
 * sgpr_score_pair_list: d_score[p] = SG-tail(d_pooled_rows[idx1[p]], d_pooled_cols[idx2[p]]) for the P pairs of the plan
 * (d_plan: the plan words in DEVICE memory; R, M, n_rows, n_items and P are the values sgpr_pair_plan was given and
 * returned - the kernels trust the plan's indices, as sgpr_score_pairs trusts idx1 / idx2).  Workspace:
 * sgpr_score_pair_list_workspace_bytes(h, n_rows, M).  A NaN or +-inf in a listed row graph or in ANY of the M column
 * graphs puts the whole list on the exact fp32 per-pair path; every pair of a NaN graph scores NaN (sgpr_score_pairs). */
size_t sgpr_pair_plan_ints(int64_t P, int R);
int sgpr_pair_plan(const int32_t* h_idx1, const int32_t* h_idx2, int64_t P, int R, int M, int32_t* h_plan,
                   size_t plan_capacity_ints, size_t* plan_ints, int32_t* n_rows, int32_t* n_items);
size_t sgpr_score_pair_list_workspace_bytes(const sgpr_handle* h, int n_rows, int M);
int sgpr_score_pair_list(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         const int32_t* d_plan, int n_rows, int n_items, int64_t P, float* d_score, void* d_workspace,
                         size_t workspace_bytes, void* stream);

/* Dense all-pairs form of the same tail: score[r, c] = SG-tail(rows[r], cols[c])
 * (the NTN is asymmetric, layers_batch.py:77-83, so the full rectangle is computed).
 * d_score is [R, ld] with ld >= M.  Workspace: sgpr_score_all_pairs_workspace_bytes.
 * A NaN or +-inf pooled vector among the rows or columns puts the whole rectangle on the exact fp32 per-pair path (like
 * inputs beyond the f16 range, on every handle kind): row r and column c of a NaN graph are NaN, every other entry is
 * within the exact path's error of the reference (sgpr_score_pairs states the rule). */
size_t sgpr_score_all_pairs_workspace_bytes(const sgpr_handle* h, int R, int M);
int sgpr_score_all_pairs(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols,
                         int M, float* d_score, int64_t ld, void* d_workspace, size_t workspace_bytes,
                         void* stream);

/* Several independent rectangles with ONE pair of launches - the matrices of the sequences of an evaluation job
 * (eval_batch.py:26-36 loops over `eva_batch.sequences`): the work items of all jobs form one list that the workgroups
 * split evenly, so small matrices do not leave the GPU half empty and the launch gaps between them disappear.  `jobs` is
 * a HOST array (its device pointers are read at launch); results are bit-identical to one sgpr_score_all_pairs per job,
 * NaN entries of a job with a non-finite pooled vector included (that job alone takes the exact path). */
#define SGPR_MAX_PAIR_JOBS 8
typedef struct sgpr_pairs_job {
    const float* d_pooled_rows;   /* [R][32] */
    int R;
    const float* d_pooled_cols;   /* [M][32] */
    int M;
    float* d_score;               /* [R][ld] */
    int64_t ld;
} sgpr_pairs_job;
size_t sgpr_score_all_pairs_multi_workspace_bytes(const sgpr_handle* h, int n_jobs, const sgpr_pairs_job* jobs);
int sgpr_score_all_pairs_multi(const sgpr_handle* h, int n_jobs, const sgpr_pairs_job* jobs, void* d_workspace,
                               size_t workspace_bytes, void* stream);

/* Drop-in SG.forward (sg_net.py:112-138): dense features of both sides in,
 * (score [B], att1 [B,N], att2 [B,N]) out; att pointers may be NULL. */
size_t sgpr_forward_workspace_bytes(const sgpr_handle* h, int B, int N, int k);
int sgpr_forward_dense(const sgpr_handle* h, const float* d_features_1, const float* d_features_2, int B, int N,
                       int k, float* d_score, float* d_att1, float* d_att2, void* d_workspace,
                       size_t workspace_bytes, void* stream);

/* Synchronises `stream` and returns SGPR_E_LABEL if any launch on this handle
 * saw a label outside [-1, num_labels) since the last check (the reference
 * raises KeyError at sg_net.py:277), else SGPR_OK.  Clears the flag.  The flags
 * are the handle's: a launch on another stream or thread raises them too, and
 * only the work of `stream` is waited for. */
int sgpr_check_status(const sgpr_handle* h, void* stream);

/* ---- consumers of the score matrix that keep it on the device ----------------------------------------
 *
 * sgpr_pair_positives + sgpr_pair_threshold_counts: the counting half of eval_batch.py:48-49 and 69-87 (sklearn roc_curve
 * / auc and precision_recall_curve -> F1 max) on an R x M score rectangle (rows row0 .. row0+R-1 of the square matrix).
 * Ground truth comes from the planar poses d_pose_xz [.][2] (float64 x, z of the KITTI pose; the distance is evaluated
 * in float64 operation by operation like utils.py:36): distance <= d_pos positive, >= d_neg negative, in between
 * ignored (the pairs the reference refuses, sg_net.py:302-309) - or, when d_pose_xz is NULL, from explicit labels
 * d_gt [R][ldg] (1 / 0 / negative = ignore).
 *
 * sgpr_pair_positives appends the scores of the positive pairs to d_out (at most `capacity` of them, in no particular
 * order; capacity 0 / d_out NULL = count only) and sets d_count[0] = number of positive pairs with a usable score,
 * d_count[1] = positive pairs whose score is negative or NaN (no defined rank; they are skipped).
 *
 * sgpr_pair_threshold_counts streams the rectangle once and counts the NEGATIVE pairs by threshold bucket: for T <=
 * 8191 ascending thresholds, d_out[b] (uint64, b = 0..T) = negatives with exactly b thresholds <= their score, so
 * FP(score >= threshold q) = sum of d_out[b], b > q.  d_out[T+1] = negatives skipped for a negative / NaN score.
 * With d_rank every negative is also ranked among ALL distinct scores of positive pairs: the thresholds are every S-th
 * of those ascending values, and d_rank holds, for threshold q, the S values from it up to the next threshold in
 * groups_per_threshold records of eight (padded with +inf / 0 pairs) together with the number of pairs that carry each;
 * d_at_least[q] = positive pairs with a score >= threshold q.  d_out[T+2] = sum over negatives of 2 #{positive pairs
 * > s} + #{positive pairs == s} = 2 P N AUC (the Mann-Whitney form of sklearn's trapezoid area): the ROC area exactly,
 * in the same pass.
 * F1 peaks at the score of a positive pair, so the host (sg_pr_amd/metrics.py) takes every S-th distinct positive value
 * as thresholds, reads exact F1 there and bounds in between, and settles the few segments that can still hold the
 * maximum with a second call - exact, no sort of the matrix, which never leaves the GPU.  The workspace holds one
 * slab of counters per workgroup (no global atomics). */
typedef struct sgpr_rank_group {
    float value[8];             /* ascending distinct scores of positive pairs (+inf padding) */
    uint32_t pairs[8];          /* positive pairs with exactly that score (0 for padding) */
} sgpr_rank_group;
int sgpr_pair_positives(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int row0,
                        const double* d_pose_xz, double d_pos, double d_neg, const signed char* d_gt, int64_t ldg,
                        float* d_out, int64_t capacity, unsigned long long* d_count, void* stream);
size_t sgpr_pair_threshold_counts_workspace_bytes(const sgpr_handle* h, int T);
int sgpr_pair_threshold_counts(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int row0,
                               const double* d_pose_xz, double d_pos, double d_neg, const signed char* d_gt,
                               int64_t ldg, const float* d_thresholds, int T, const sgpr_rank_group* d_rank,
                               int groups_per_threshold, const unsigned long long* d_at_least, unsigned long long* d_out,
                               void* d_workspace, size_t workspace_bytes, void* stream);

/* F1-max of a score rectangle (eval_batch.py:69, 85-87) in ONE call, no host round trip between its steps: one
 * streaming pass classifies every pair once - negatives into a histogram over the score's bit pattern (one shift, one LDS
 * atomic), the scores of the positive pairs into a list -, exact F1 at every bin edge and bounds for the positives
 * inside the bins follow from suffix sums, and a second pass settles the few bins that can still hold the maximum
 * (their positives sorted and de-duplicated in LDS; a negative outside them costs one bit test).  Same ground truth
 * arguments as sgpr_pair_positives.  d_result (device, 8 doubles): [0] F1-max (exact), [1] status - 0 ok, 1 the
 * rectangle needs the multi-call path (more than 2^20 positive pairs, or more than 4095 positive scores left to settle:
 * a flat curve), 2 negative / NaN scores among the labelled pairs -, [2] positive pairs, [3] negative pairs, [4] passes
 * over the matrix, [5] bins of the first pass, [6] values settled by the second.  Asynchronous on `stream`; the caller
 * copies d_result when it needs it. */
size_t sgpr_f1_max_workspace_bytes(const sgpr_handle* h, int R, int M);
int sgpr_f1_max(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int row0, const double* d_pose_xz,
                double d_pos, double d_neg, const signed char* d_gt, int64_t ldg, double* d_result, void* d_workspace,
                size_t workspace_bytes, void* stream);

/* Loop-closure candidates (the use the reference makes of a sequence's similarity matrix, README.md:92-97): for every
 * row r the k (1, 4, 8 or 16) best-scoring columns c with |c - (row0 + r)| > window (window = -1 keeps every column),
 * ordered by (score descending, column ascending); d_values / d_indices [R][k], index -1 where fewer than k columns
 * qualify.  One wave per row, one pass over the row. */
int sgpr_topk_rows(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int row0, int window, int k,
                   float* d_values, int32_t* d_indices, void* stream);

/* Loop-closure candidates straight from pooled vectors, without the R x M matrix: for every row r the k (1..16)
 * best-scoring columns c of the rectangle d_pooled_rows [R] x d_pooled_cols [M], in sgpr_topk_rows' order and with its
 * rules (score descending, column ascending; NaN never qualifies; (-inf, -1) where fewer than k columns qualify).  Column
 * c qualifies for row r iff |c - self_r| > window (window < 0: no window) and, with SGPR_TOPK_CAUSAL in flags, c < self_r,
 * where self_r = d_row_self[r] (device, [R], each in [0, M): sgpr_check_status reports an entry outside) or, with
 * d_row_self NULL, row0 + r.  Every value is bit-identical to sgpr_score_all_pairs' entry at (r, c) on the same
 * rectangle.  The production handle runs one fused launch (the all-pairs tail feeding per-row lists) plus a small merge
 * launch; its workspace grows with R + M, never with R * M.  Wide-range and any-shape handles score row blocks of at
 * most 64 MB with their own tail and select from each.  Wherever a call runs in row blocks, the f16-range question is
 * answered once per call, over the whole rectangle, before its first block: every block takes the datapath
 * sgpr_score_all_pairs takes on that rectangle.  d_values / d_indices [R][k], device.  Arguments are checked
 * before the device is touched: a NULL pointer, k outside 1..16 or unknown flag bits give SGPR_E_INVALID, a workspace
 * below sgpr_score_topk_workspace_bytes SGPR_E_WORKSPACE.  Asynchronous on `stream`.
 * A row graph whose pooled vector holds a NaN gets (-inf, -1) in every slot and a NaN column graph is never listed: their
 * scores are NaN (sgpr_score_pairs).  The same holds for sgpr_score_topk_large and sgpr_score_seq_topk below. */
#define SGPR_TOPK_CAUSAL 1
size_t sgpr_score_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags);
int sgpr_score_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                    const int32_t* d_row_self, int row0, int window, int flags, int k, float* d_values,
                    int32_t* d_indices, void* d_workspace, size_t workspace_bytes, void* stream);

/* Loop-closure candidates for k up to SGPR_TOPK_LARGE_MAX (recall@1 %, candidate lists for a geometric check).  Same
 * lists as sgpr_score_topk / sgpr_topk_rows: for every row r the k best eligible columns by (value descending, column
 * ascending), IEEE comparison (-0.0 ties +0.0, the lower column first; the stored bits are reported), NaN and -inf never
 * qualify, (-inf, -1) in the slots past the last qualifying column (k > M is allowed).  Eligibility is sgpr_score_topk's:
 * |c - self_r| > window (window < 0: no window), with SGPR_TOPK_CAUSAL c < self_r, self_r = d_row_self[r] or row0 + r
 * (an entry of d_row_self outside [0, M): sgpr_check_status reports it).  For k <= 16 both return the bits and indices
 * of the k <= 16 entry points.
 * - sgpr_topk_rows_large: a resident matrix d_score [R][ld] (ld >= M, window >= -1, as sgpr_topk_rows).
 * - sgpr_score_topk_large: the rectangle d_pooled_rows [R] x d_pooled_cols [M] scored in row blocks of at most 64 MB
 *   (every handle), each selected as it is written; every value is sgpr_score_all_pairs' entry on the whole rectangle
 *   (the f16-range question is answered once per call).
 * A radix select over order-preserving keys, each row split across workgroups (sgpr_select.hip).
 * Workspace: one 64 MB score block (pooled form) plus terms linear in min(R, 4096) and M, never R * M.  Arguments are
 * checked before the device is touched: a NULL pointer, k outside 1..SGPR_TOPK_LARGE_MAX, unknown flag bits or
 * row0 + R past INT_MAX give SGPR_E_INVALID, a workspace below the _workspace_bytes answer SGPR_E_WORKSPACE (which is
 * 0 for invalid arguments).  Results depend on the arguments alone, never on the workspace's contents.  Asynchronous
 * on `stream`. */
#define SGPR_TOPK_LARGE_MAX 4096
size_t sgpr_topk_rows_large_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags);
int sgpr_topk_rows_large(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const int32_t* d_row_self,
                         int row0, int window, int flags, int k, float* d_values, int32_t* d_indices, void* d_workspace,
                         size_t workspace_bytes, void* stream);
size_t sgpr_score_topk_large_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags);
int sgpr_score_topk_large(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                          const int32_t* d_row_self, int row0, int window, int flags, int k, float* d_values,
                          int32_t* d_indices, void* d_workspace, size_t workspace_bytes, void* stream);

/* Sequence-matched loop closures: a score averaged along a diagonal of the similarity matrix.  Rows and columns are
 * consecutive scans of a trajectory (row r - 1 is the scan before row r; the columns are ONE trajectory).  A revisited
 * place is a run of good scores along c - r = const (driven the same way, SGPR_SEQ_FORWARD) or c + r = const (driven the
 * opposite way, SGPR_SEQ_REVERSE).  For a sequence length L in 1..SGPR_SEQ_MAX_LEN and sigma = +1 forward, -1 reverse:
 *     D(r, c)      = { d in 0..L-1 : r - d >= 0 and 0 <= c - sigma d < M }       (d = 0 is always in it)
 *     Q_sigma[r,c] = (S[r, c] + S[r-1, c-sigma] + ...) * rcp[|D|],               rcp[n] = (float)(1.0 / n)
 * plain fp32 additions in ascending d starting from the d = 0 term, one fp32 multiplication, nothing fused: reproducible
 * bit for bit.  Both flags: Q = Q_reverse and dir = 1 where Q_reverse > Q_forward or Q_forward is NaN, else Q = Q_forward
 * and dir = 0 (forward wins ties); one flag: dir is that direction (0 forward, 1 reverse) everywhere.  NaN and +-inf terms
 * propagate by IEEE rules.  Terms are never masked: the window applies to the end point (r, c) alone, and
 * window >= 2 (L - 1) keeps the self diagonal c = r out of every reverse sum of an eligible end point.  The first `ctx`
 * rows are context only: outputs exist for rows ctx .. R-1 at output row r - ctx (ctx == R: an empty result).
 * - sgpr_seq_filter: a resident matrix d_score [R][ld] -> d_out [R - ctx][ldo] (ld, ldo >= M) and, unless NULL, d_dir
 *   u8 [R - ctx][ldo].  Out of place: d_out overlapping d_score is undefined.  No workspace.
 * - sgpr_score_seq_topk: the rectangle d_pooled_rows [R] x d_pooled_cols [M] on any handle, scored in row blocks; for
 *   every row r >= ctx the k (1..SGPR_TOPK_LARGE_MAX) best eligible columns by Q, in sgpr_topk_rows_large's order and with
 *   its padding and NaN rules (a NaN Q never qualifies) -> d_values / d_indices [R - ctx][k] and, unless NULL, d_dirs u8
 *   [R - ctx][k]: the direction of each listed Q, 0 in a padding slot.  Eligibility is sgpr_score_topk's on (r, c):
 *   window, SGPR_TOPK_CAUSAL, self_r = d_row_self[r] (device, [R]: context rows have entries too) or row0 + r, r counted
 *   over all R rows.  Every S term is sgpr_score_all_pairs' entry on the whole rectangle (the f16-range question is
 *   answered once per call).  A score block holds at most 64 MB including L - 1 context rows, so a block yields
 *   max(1, 64 MB / 4M - (L - 1)) output rows; its last L - 1 rows become the next block's context by a device-to-device
 *   copy and are not scored again.  Workspace: that block, a Q block (and a dir block with both directions) of the same
 *   rows, the selection's, the all-pairs tail's: linear in M and min(R, block rows), never R * M.
 * Arguments are checked before the device is touched: a NULL pointer, L outside 1..SGPR_SEQ_MAX_LEN, ctx outside 0..R, no
 * direction flag, unknown flag bits, k outside 1..SGPR_TOPK_LARGE_MAX or row0 + R past INT_MAX give SGPR_E_INVALID, a
 * workspace below the _workspace_bytes answer SGPR_E_WORKSPACE (which is 0 for invalid arguments).  Results depend on the
 * arguments alone.  Asynchronous on `stream`. */
#define SGPR_SEQ_FORWARD 2
#define SGPR_SEQ_REVERSE 4
#define SGPR_SEQ_MAX_LEN 32
int sgpr_seq_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx, int L, int flags,
                    float* d_out, int64_t ldo, unsigned char* d_dir, void* stream);
size_t sgpr_score_seq_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int k, int flags);
int sgpr_score_seq_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                        int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L, int k,
                        float* d_values, int32_t* d_indices, unsigned char* d_dirs, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* Distinct-place loop closures: per-row score peaks within a scan radius.  A trajectory revisits a place over many
 * consecutive scans, so the k best columns of a row are mostly one place seen k times.  With X the ranked score (S of
 * sgpr_score_all_pairs, or Q above), a column QUALIFIES for row r iff it is eligible (sgpr_score_topk's rule: window,
 * SGPR_TOPK_CAUSAL, self_r = d_row_self[r] or row0 + r) and X[r, c] is neither NaN nor -inf (+inf qualifies);
 * qualifying columns are ordered as sgpr_topk_rows_large lists them (value descending by IEEE comparison, -0.0 ties
 * +0.0, then column ascending).  For a radius rho in 0..SGPR_PEAK_MAX_RADIUS:
 *     column c is a PEAK of row r iff it qualifies and it comes first, in that order, among the qualifying columns c'
 *     with |c' - c| <= rho.
 * - Two peaks of a row are more than rho columns apart; the best qualifying column of a row is always a peak; rho = 0
 *   makes every qualifying column a peak.
 * - A column that does not qualify (ineligible, NaN, -inf) neither is a peak nor suppresses anything.  A causal query
 *   that knows only the columns c < self_r therefore gets the lists of the offline call.  The first eligible column
 *   beside an excluded window can be a peak of a slope that rises into the window: choose rho <= window.
 * - On a plateau of equal values longer than rho only its first column is a peak ("first in its neighbourhood", not
 *   "not beaten by a peak").
 * - Each row is independent of every other row, and nothing depends on an evaluation order.
 * - sgpr_peak_filter: a resident block d_score [R][ld] -> d_out [R][ldo] (ld, ldo >= M): X[r, c] (the stored bits) at
 *   a peak, -inf elsewhere; every entry of [R][M] is written, nothing beyond column M.  Out of place: d_out overlapping
 *   d_score is undefined.  No workspace.  One workgroup per strip of SGPR_PEAK_STRIP columns of a row (sgpr_peak.hip,
 *   DESIGN.md §20).  An entry of d_row_self outside [0, M) only moves the window; the selections report it.
 * - sgpr_score_peak_topk: sgpr_score_seq_topk's arguments and rules (a direction flag is required, the first ctx rows
 *   are context only, d_dirs may be NULL, every handle, row blocks of at most 64 MB, the f16-range question answered
 *   once per call) plus `radius`: for every row r >= ctx the k (1..SGPR_TOPK_LARGE_MAX) best PEAKS of Q (L = 1: of S
 *   itself) in list order, (-inf, -1) in the slots past the last peak.  Each block is scored, filtered along the
 *   diagonals (L > 1), peak-filtered into a P block and selected from it; the workspace is sgpr_score_seq_topk's plus
 *   that P block, never R * M.  radius = 0 returns the bits of sgpr_score_seq_topk.
 * Arguments are checked before the device is touched: sgpr_score_seq_topk's, and a radius outside
 * 0..SGPR_PEAK_MAX_RADIUS gives SGPR_E_INVALID; a workspace below the _workspace_bytes answer SGPR_E_WORKSPACE (which is
 * 0 for invalid arguments).  R == ctx or M == 0 writes padding lists without scoring.  Results depend on the arguments
 * alone.  Asynchronous on `stream`. */
#define SGPR_PEAK_MAX_RADIUS 1024
#define SGPR_PEAK_STRIP 1024
int sgpr_peak_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const int32_t* d_row_self,
                     int row0, int window, int flags, int radius, float* d_out, int64_t ldo, void* stream);
size_t sgpr_score_peak_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int k, int radius,
                                            int flags);
int sgpr_score_peak_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L, int radius, int k,
                         float* d_values, int32_t* d_indices, unsigned char* d_dirs, void* d_workspace,
                         size_t workspace_bytes, void* stream);

/* Speed-tolerant sequence matching: the diagonal mean of sgpr_seq_filter, maximised over a set of paths.  Scans are
 * sampled in time, not in distance: a revisit driven at another speed, or matched against a keyframe-thinned map, is a
 * line of slope p/q != 1, on which the unit diagonal averages one true score with L - 1 unrelated ones.
 * A PATH is off[0..L-1], int32, with off[0] = 0, non-decreasing, off[L-1] <= SGPR_SEQ_PATH_MAX_OFFSET: the column
 * distance walked back after d row steps.  A call takes n_paths paths, 1..SGPR_SEQ_MAX_PATHS, as a HOST array
 * h_offsets [n_paths][L]; the array is copied into the launch and is free to reuse after the call returns.
 * For path p and sigma = +1 (SGPR_SEQ_FORWARD) or -1 (SGPR_SEQ_REVERSE):
 *     D_p(r, c)    = { d in 0..L-1 : r - d >= 0 and 0 <= c - sigma off_p[d] < M }     (a prefix: off is monotone)
 *     Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|],       rcp[n] = (float)(1.0 / n)
 * plain fp32 additions in ascending d starting from the d = 0 term, one fp32 multiplication, nothing fused; terms are
 * never masked and never replaced by zero.  The result is a fold over the candidates in this order: forward paths
 * 0..n_paths-1, then reverse paths 0..n_paths-1 (directions not asked for are skipped).  `best` starts as the first
 * candidate; a later x replaces it iff x > best or best is NaN; code (u8) = direction bit | path << 1 of the winner.
 * With the single path off[d] = d this is sgpr_seq_filter bit for bit and code is its dir.  Duplicate paths are allowed
 * and change nothing.  Everything else is sgpr_seq_filter's: the context rows ctx, eligibility on the end point only,
 * NaN / inf propagation, 1 <= L <= SGPR_SEQ_MAX_LEN.
 * - window >= L - 1 + the largest offset keeps the self diagonal out of every sum of an eligible end point.
 * - A streaming place database (rows arrive one at a time, columns are the frames stored so far) gets the offline lists
 *   iff window >= the largest offset; otherwise a reverse sum of an eligible column reaches a frame not stored yet.
 * - sgpr_seq_path_filter: a resident matrix d_score [R][ld] -> d_out [R - ctx][ldo] and, unless NULL, d_code u8
 *   [R - ctx][ldo].  Out of place.  No workspace.  One workgroup per tile of 32 rows x 256 columns with a halo of the
 *   call's largest offset (seq_path_kernel in sgpr_seq.hip).
 * - sgpr_score_path_topk: sgpr_score_peak_topk's structure (row blocks with L - 1 context rows, the f16-range question
 *   answered once per call, every handle) with the path filter in place of the diagonal filter; the peak step runs only
 *   when radius > 0.  d_codes u8 [R - ctx][k] (or NULL): the code of each listed entry, 0 in a padding slot.  With the
 *   unit path the lists are the bits of sgpr_score_seq_topk (radius 0) / sgpr_score_peak_topk (radius > 0) and the
 *   workspace equals theirs; with n_paths > 1 and one direction it grows by one code block of the block's rows x M
 *   bytes.  Never R * M.
 * Arguments are checked before the device is touched: those of the calls above, and n_paths outside
 * 1..SGPR_SEQ_MAX_PATHS, a NULL table, off[p][0] != 0, a decreasing step or an offset above SGPR_SEQ_PATH_MAX_OFFSET give
 * SGPR_E_INVALID with a message naming the fault (the workspace answer is 0 for invalid arguments).  R == ctx or M == 0
 * writes padding lists without scoring.  Results depend on the arguments alone.  Asynchronous on `stream`. */
#define SGPR_SEQ_MAX_PATHS 16
#define SGPR_SEQ_PATH_MAX_OFFSET 64
int sgpr_seq_path_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx, int L, int flags,
                         const int32_t* h_offsets, int n_paths, float* d_out, int64_t ldo, unsigned char* d_code,
                         void* stream);
size_t sgpr_score_path_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int n_paths, int k,
                                            int radius, int flags);
int sgpr_score_path_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L,
                         const int32_t* h_offsets, int n_paths, int radius, int k, float* d_values, int32_t* d_indices,
                         unsigned char* d_codes, void* d_workspace, size_t workspace_bytes, void* stream);

/* Multi-session maps: the path-set mean above where the rows and the columns are SEVERAL trajectories (sessions: a map
 * recorded on earlier drives, then the current drive), stacked in time order.  Every call above takes the columns for one
 * trajectory; on a stacked map its index window hides the true matches of a session that starts where the one before
 * ended, and its diagonals average across the seam.  Here sums and the window stop at session boundaries.
 * A SESSION TABLE is a HOST array starts[0..n-1], int32: starts[0] = 0, non-decreasing (a repeated value is an empty
 * session), every value <= R (row table) or <= M (column table), n in 1..SGPR_SESSION_MAX; NULL with n = 0 means one
 * session.  The arrays are copied into the launch and are free to reuse after the call returns.
 *     sess(x) = the largest j with starts[j] <= x; an index below 0 counts as session 0 (an index at or past the end
 *               falls, by the same rule, into the last session)
 *     lo(x), hi(x) = the first and the last index of session sess(x): starts[j] and starts[j + 1] - 1 (the last session
 *               ends at R - 1 / M - 1)
 * For path p (sgpr_seq_path_filter's table; NULL with n_paths = 0 is the unit diagonal off[d] = d) and sigma = +1 / -1:
 *     D_p(r, c)    = { d in 0..L-1 : r - d >= lo_row(r) and lo_col(c) <= c - sigma off_p[d] <= hi_col(c) }   (a prefix)
 *     Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|]
 * Additions, the multiplication, the fold over the candidates, `code`, the context rows and NaN / inf propagation are
 * sgpr_seq_path_filter's, bit for bit.
 * SESSION WINDOW: with window >= 0, column c is excluded for row r iff sess_col(c) == sess_col(self_r) and
 * |c - self_r| <= window, self_r = d_row_self[r] (device, [R]: context rows have entries too) or, d_row_self NULL,
 * row0 + r.  Columns of other sessions are never window-excluded; terms are never masked.  SGPR_TOPK_CAUSAL keeps its
 * meaning, c < self_r: sessions are stacked in time order, so every earlier session is visible.
 * Identities: (1) one row session, one column session, window = -1: sgpr_seq_path_filter's bits and codes; (2) one
 * session each, any window: the pooled call's lists are sgpr_score_path_topk's with radius = 0; (3) window = -1: the
 * block Q[rows of row session i, columns of column session j] is sgpr_seq_path_filter run on that sub-matrix alone, a row
 * session's context rows being the rows of that session before the block.
 * - sgpr_session_filter: a resident matrix d_score [R][ld] -> d_out [R - ctx][ldo] and, unless NULL, d_code u8
 *   [R - ctx][ldo]; an excluded end point gets -inf with code 0.  Out of place.  No workspace.  The causal flag is not
 *   accepted (the pooled call hands it to its selection).  sgpr_seq_path_filter's tile and halo (session_kernel in sgpr_seq.hip,
 *   DESIGN.md §22).
 * - sgpr_score_session_topk: sgpr_score_path_topk's arguments without `radius`, plus the two tables, and its structure
 *   (row blocks with L - 1 context rows, the f16-range question answered once per call, every handle): the session filter
 *   in place of the path filter with the row table shifted per block, then the large-k selection without a window (an
 *   excluded end point is -inf and never listed).  The workspace equals sgpr_score_path_topk_workspace_bytes at
 *   radius = 0 (n_paths = 0 counting as one path).
 * Arguments are checked before the device is touched: those of sgpr_seq_path_filter / sgpr_score_path_topk, a window
 * below -1, and a table that does not start at 0, decreases, has an entry past its limit, n outside
 * 0..SGPR_SESSION_MAX, NULL with n > 0 (or a table with n = 0), a path table with n_paths = 0 give SGPR_E_INVALID with a
 * message naming the fault (the workspace answer is 0 for invalid arguments).  R == ctx or M == 0 writes padding lists
 * without scoring.  Results depend on the arguments alone.  Asynchronous on `stream`. */
#define SGPR_SESSION_MAX 64
int sgpr_session_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx, int L, int flags,
                        const int32_t* h_offsets, int n_paths, const int32_t* h_row_starts, int n_row_sessions,
                        const int32_t* h_col_starts, int n_col_sessions, const int32_t* d_row_self, int row0, int window,
                        float* d_out, int64_t ldo, unsigned char* d_code, void* stream);
size_t sgpr_score_session_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int n_paths, int k,
                                               int flags, int n_row_sessions, int n_col_sessions);
int sgpr_score_session_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                            int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L,
                            const int32_t* h_offsets, int n_paths, const int32_t* h_row_starts, int n_row_sessions,
                            const int32_t* h_col_starts, int n_col_sessions, int k, float* d_values, int32_t* d_indices,
                            unsigned char* d_codes, void* d_workspace, size_t workspace_bytes, void* stream);

/* Hard-pair mining without the R x M matrix: for every row r the k (1..16) hardest pose-labelled pairs (r, c) of the
 * rectangle d_pooled_rows [R] x d_pooled_cols [M].
 * - Column c is eligible for row r iff it is for sgpr_score_topk (window, SGPR_TOPK_CAUSAL, self_r = d_row_self[r] or
 *   row0 + r), c != self_r, and the pair's pose class is the one flags ask for.  The class is sgpr_pair_positives'
 *   float64 rule on the row pose and d_col_pose_xz[c] (device, [M][2] x, z): the row pose is d_row_pose_xz[r] (device,
 *   [R][2]) or, with d_row_pose_xz NULL, d_col_pose_xz[self_r] (none when self_r lies outside [0, M): the row gets
 *   nothing).
 * - SGPR_MINE_NEGATIVES: distance >= d_neg, score descending, then column ascending (-inf, -1 in empty slots) - the
 *   perceptual aliases a back end must reject.  SGPR_MINE_POSITIVES: distance <= d_pos, score ascending, then column
 *   ascending (+inf, -1 in empty slots) - the missed revisits.  Exactly one of the two is set.
 * - A NaN score or a NaN pose never qualifies.  Every value is bit-identical to sgpr_score_all_pairs' entry (r, c); two
 *   calls return identical bytes.
 * - The production handle runs sgpr_score_topk's fused launch with the pose test in its epilogue: a 256-column chunk
 *   whose pose box lies beyond d_pos of the wave's rows is not scored at all for the positives, and one beyond
 *   max(d_pos, d_neg) needs no per-pair arithmetic for the negatives.  Its workspace grows with R + M, never R * M.
 *   Wide-range and any-shape handles score row blocks of at most 64 MB with their own tail and run sgpr_mine_rows on
 *   each; the f16 range is decided once per call, as for sgpr_score_topk.
 * d_values / d_indices [R][k], device.  Arguments are checked before the device is touched: a NULL handle, pooled
 * array, column pose array or output, k outside 1..16, zero or both mode flags or unknown bits, a NaN d_pos / d_neg,
 * d_pos < 0, d_pos > d_neg or row0 + R beyond an int give SGPR_E_INVALID, a workspace below sgpr_score_mine_workspace_bytes
 * SGPR_E_WORKSPACE; a d_row_self entry outside [0, M) is reported by sgpr_check_status.  Asynchronous on `stream`.
 * A graph whose pooled vector holds a NaN is never mined, as a row (empty slots) or as a column: its scores are NaN. */
#define SGPR_MINE_NEGATIVES 2
#define SGPR_MINE_POSITIVES 4
size_t sgpr_score_mine_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags);
int sgpr_score_mine(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                    const double* d_col_pose_xz, const double* d_row_pose_xz, const int32_t* d_row_self, int row0,
                    int window, int flags, double d_pos, double d_neg, int k, float* d_values, int32_t* d_indices,
                    void* d_workspace, size_t workspace_bytes, void* stream);

/* sgpr_score_mine's selection on a resident matrix d_score [R][ld] (ld >= M), with its rules, flags, checks and order:
 * one wave per row, one pass over the row.  Needs no workspace (sgpr_mine_rows_workspace_bytes returns 0; the
 * arguments are kept for later use). */
size_t sgpr_mine_rows_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags);
int sgpr_mine_rows(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const double* d_col_pose_xz,
                   const double* d_row_pose_xz, const int32_t* d_row_self, int row0, int window, int flags, double d_pos,
                   double d_neg, int k, float* d_values, int32_t* d_indices, void* d_workspace, size_t workspace_bytes,
                   void* stream);

/* Range retrieval without the R x M matrix: every eligible pair (r, c) of the rectangle d_pooled_rows [R] x
 * d_pooled_cols [M] whose score is >= threshold.
 * - Eligibility is sgpr_score_topk's: |c - self_r| > window (window < 0: no window) and, with SGPR_TOPK_CAUSAL in flags,
 *   c < self_r, where self_r = d_row_self[r] (device, [R], each in [0, M): sgpr_check_status reports an entry outside)
 *   or, with d_row_self NULL, row0 + r.  A NaN score never qualifies; threshold = -inf takes every non-NaN eligible pair.
 * - Every value is bit-identical to sgpr_score_all_pairs' entry (r, c) on the same rectangle and handle (every handle
 *   kind, both sides of the f16 range guard).
 * - Order: row-major (r ascending, then c ascending), independent of grid, occupancy and timing: two calls return
 *   identical bytes.
 * - *d_count (device, 64-bit) receives the exact number of qualifying pairs; d_row_ptr (device [R + 1] int64, may be
 *   NULL) its CSR row pointer: row_ptr[0] = 0, row_ptr[R] = count.  Only the first min(count, capacity) pairs in that
 *   order are written to d_rows / d_cols (int32) and d_values (f32), device [capacity].  capacity = 0 with NULL arrays
 *   counts only.  M = 0 gives count 0 and an all-zero row_ptr.  Positions are 64-bit: R * M may exceed 2^31.
 * - Checked before the device is touched (SGPR_E_INVALID): a NULL handle, d_count or pooled vector (R, M > 0), a negative
 *   count or capacity, capacity > 0 with a NULL output array, unknown flag bits, a NaN threshold, row0 + R beyond an
 *   int.  A workspace below sgpr_score_above_workspace_bytes is SGPR_E_WORKSPACE.
 * - The production handle runs two passes of one fused instance of the all-pairs tail (count, then write the flagged
 *   work items) around a small fold + scan; its workspace grows with R + M and the grid, never with R * M (the operands,
 *   O(R) counters and row pointers, O(grid) partial counts, one byte per 16 x 256 work item).  Wide-range and any-shape
 *   handles score row blocks of at most 64 MB with their own tail and select from each with sgpr_rows_above's kernels,
 *   positions continuing on the device.  The production handle's launches take at most 131 072 rows each; on every
 *   handle the f16 range of a row-blocked call is decided once, over the whole rectangle.  Asynchronous on `stream`, no host synchronisation inside.
 *   A pair of a graph whose pooled vector holds a NaN is never listed (its score is NaN, sgpr_score_pairs): at
 *   threshold -inf exactly the pairs of two NaN-free graphs come back.  The same holds for sgpr_score_seq_above, where a
 *   NaN score makes every Q whose diagonals all run through it NaN. */
size_t sgpr_score_above_workspace_bytes(const sgpr_handle* h, int R, int M, int flags);
int sgpr_score_above(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                     const int32_t* d_row_self, int row0, int window, int flags, float threshold,
                     int32_t* d_rows, int32_t* d_cols, float* d_values, int64_t capacity,
                     int64_t* d_row_ptr, unsigned long long* d_count,
                     void* d_workspace, size_t workspace_bytes, void* stream);

/* sgpr_score_above's selection, contract and checks on a resident matrix d_score [R][ld] (ld >= M; NULL with R or M
 * zero): the same pairs, order and counts (a NULL d_score with R, M > 0 or ld < M is SGPR_E_INVALID).  Workspace
 * O(R). */
size_t sgpr_rows_above_workspace_bytes(const sgpr_handle* h, int R, int M);
int sgpr_rows_above(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld,
                    const int32_t* d_row_self, int row0, int window, int flags, float threshold,
                    int32_t* d_rows, int32_t* d_cols, float* d_values, int64_t capacity,
                    int64_t* d_row_ptr, unsigned long long* d_count,
                    void* d_workspace, size_t workspace_bytes, void* stream);

/* Whole-sequence evaluation without the R x M matrix: sgpr_pair_positives and sgpr_pair_threshold_counts on the
 * rectangle d_pooled_rows [R] x d_pooled_cols [M] that sgpr_score_all_pairs would write, scored as they go and never
 * stored.  Ground truth arguments (d_pose_xz / d_pos / d_neg or d_gt [R][ldg], row0) and outputs are exactly those of the
 * matrix versions.
 * - sgpr_score_positives: the same multiset of positive scores as sgpr_pair_positives on that matrix, bit for bit
 *   (unordered, the first `capacity` of them written), and the same d_count[0..1].
 * - sgpr_score_threshold_counts: d_out[0..T+2] equal to sgpr_pair_threshold_counts' on that matrix (bucket counts, the
 *   skipped negative / NaN count, the rank sum).  T <= SGPR_SCORE_COUNT_MAX_THRESHOLDS (2047: the threshold tree,
 *   counters and ranking table of a workgroup live in 32 KB of LDS beside the scoring tail); a larger T is
 *   SGPR_E_INVALID.
 * - Checked before the device is touched (SGPR_E_INVALID): a NULL handle, output, ground truth or pooled vector (R, M >
 *   0), R or M < 0, row0 + R beyond an int, T out of range, a ranking without thresholds / groups / d_at_least, capacity
 *   < 0 or > 0 with a NULL d_out.  A workspace below the *_workspace_bytes query is SGPR_E_WORKSPACE.  Any workspace
 *   contents give the same result.  Asynchronous on `stream`; the caller's device is restored.
 * - Production handle: fused epilogues of the all-pairs tail.  With poses, a 16 x 256 work item whose row and column
 *   pose boxes are farther apart than d_pos is not scored by the positives pass, and one farther than max(d_pos, d_neg)
 *   is counted without per-pair float64 arithmetic.  Counting is per workgroup in 32-bit LDS counters, one slab per
 *   workgroup, folded by a small kernel; rows run in blocks of at most 131 072 and of fewer than 2^20 work items per
 *   workgroup, so no counter can overflow and any int R, M is supported (R * M < 2^62).  The workspace grows with
 *   R + M, T and the grid, never with R * M.
 * - Wide-range (debug bit 13, out-of-range weights) and any-shape handles score row blocks of at most 64 MB with their
 *   own tail and run the matrix kernels on each block, row0 advancing; the blocks' counts are summed on the device.
 * - On every handle the f16-range question of a row-blocked call is answered once, over the whole rectangle, before
 *   its first block, so the values counted are sgpr_score_all_pairs' on the same rectangle.
 * - Every labelled pair of a graph whose pooled vector holds a NaN lands in the skipped counts (d_count[1], d_out[T+1]):
 *   its score is NaN (sgpr_score_pairs). */
#define SGPR_SCORE_COUNT_MAX_THRESHOLDS 2047
size_t sgpr_score_positives_workspace_bytes(const sgpr_handle* h, int R, int M);
int sgpr_score_positives(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int row0, const double* d_pose_xz, double d_pos, double d_neg, const signed char* d_gt,
                         int64_t ldg, float* d_out, int64_t capacity, unsigned long long* d_count,
                         void* d_workspace, size_t workspace_bytes, void* stream);
size_t sgpr_score_threshold_counts_workspace_bytes(const sgpr_handle* h, int R, int M, int T);
int sgpr_score_threshold_counts(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols,
                                int M, int row0, const double* d_pose_xz, double d_pos, double d_neg,
                                const signed char* d_gt, int64_t ldg, const float* d_thresholds, int T,
                                const sgpr_rank_group* d_rank, int groups_per_threshold,
                                const unsigned long long* d_at_least, unsigned long long* d_out,
                                void* d_workspace, size_t workspace_bytes, void* stream);

/* Range retrieval and pooled evaluation on the sequence-matched score Q of sgpr_seq_filter (same D, Q, dir, ctx, L and
 * direction flags; every call reports the bits sgpr_seq_filter would write for the same S).
 * - sgpr_seq_rows_above (a resident matrix d_score [R][ld]) and sgpr_score_seq_above (the rectangle d_pooled_rows [R] x
 *   d_pooled_cols [M], every handle): every pair (r, c) with ctx <= r < R that is eligible and has Q[r, c] >= threshold.
 *   Eligibility is sgpr_score_topk's on the end point alone - self_r = d_row_self[r] (device, [R]: context rows have
 *   entries too) or row0 + r, r counted over all R rows; window and SGPR_TOPK_CAUSAL as there; terms are never masked.
 *   A NaN Q never qualifies, threshold = -inf takes every non-NaN eligible pair, a NaN threshold is SGPR_E_INVALID.
 *   Order, capacity and counts are sgpr_score_above's: row-major (r, then c ascending), two calls return identical bytes;
 *   d_rows holds the output row r - ctx, d_values the bits of Q, d_dirs (u8, may be NULL) the direction of each listed Q
 *   (the fixed direction with one flag); d_row_ptr (int64 [R - ctx + 1], may be NULL) and *d_count are exact also when
 *   `capacity` cuts the output; capacity = 0 with NULL arrays counts only.  A d_row_self entry outside [0, M) is reported
 *   by sgpr_check_status.  ctx == R, R == 0 and M == 0 are valid empty calls (count 0, all-zero row pointer).
 *   Two passes of the filter's tile kernel with a range-select epilogue (count per 64-column segment, scan, write): no
 *   Q or dir block exists.  sgpr_score_seq_above runs them on sgpr_score_seq_topk's row blocks (at most 64 MB including
 *   the L - 1 context rows, the f16-range question answered once per call), positions continuing on the device; its
 *   workspace is that block, 4 bytes per 64 columns and row of a block, O(R) counters and the all-pairs tail's.
 * - sgpr_score_seq_positives / sgpr_score_seq_threshold_counts: what sgpr_pair_positives / sgpr_pair_threshold_counts
 *   return on the matrix Q[ctx..R-1][M] - the same multiset of positives bit for bit, equal d_count[0..1] and
 *   d_out[0..T+2] - from the pooled vectors, on every handle.  With poses the row pose of output row o is
 *   d_pose_xz[row0 + ctx + o]; explicit labels d_gt are [R - ctx][ldg], indexed by output row.  flags hold direction
 *   flags only.  T <= SGPR_SCORE_COUNT_MAX_THRESHOLDS.  Each row block is filtered into a Q block of its own rows and
 *   counted by the matrix kernels; the blocks' results are added up on the device.
 * Arguments are checked before the device is touched (sgpr_score_seq_topk's, sgpr_score_above's and
 * sgpr_score_positives' rules and return codes); the _workspace_bytes queries answer 0 for invalid arguments, a workspace
 * below them is SGPR_E_WORKSPACE.  Results depend on the arguments alone.  Asynchronous on `stream`. */
size_t sgpr_seq_rows_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx);
int sgpr_seq_rows_above(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx,
                        const int32_t* d_row_self, int row0, int window, int flags, int L, float threshold,
                        int32_t* d_rows, int32_t* d_cols, float* d_values, unsigned char* d_dirs, int64_t capacity,
                        int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace, size_t workspace_bytes,
                        void* stream);
size_t sgpr_score_seq_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int flags);
int sgpr_score_seq_above(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L, float threshold,
                         int32_t* d_rows, int32_t* d_cols, float* d_values, unsigned char* d_dirs, int64_t capacity,
                         int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace, size_t workspace_bytes,
                         void* stream);
size_t sgpr_score_seq_positives_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int flags);
int sgpr_score_seq_positives(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                             int ctx, int L, int flags, int row0, const double* d_pose_xz, double d_pos, double d_neg,
                             const signed char* d_gt, int64_t ldg, float* d_out, int64_t capacity,
                             unsigned long long* d_count, void* d_workspace, size_t workspace_bytes, void* stream);
size_t sgpr_score_seq_threshold_counts_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int flags,
                                                       int T);
int sgpr_score_seq_threshold_counts(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols,
                                    int M, int ctx, int L, int flags, int row0, const double* d_pose_xz, double d_pos,
                                    double d_neg, const signed char* d_gt, int64_t ldg, const float* d_thresholds, int T,
                                    const sgpr_rank_group* d_rank, int groups_per_threshold,
                                    const unsigned long long* d_at_least, unsigned long long* d_out, void* d_workspace,
                                    size_t workspace_bytes, void* stream);

/* Thresholded closures on multi-session maps: the range retrieval of sgpr_seq_rows_above / sgpr_score_seq_above on the
 * session-aware path-set score of sgpr_session_filter, with a MINIMUM TERM COUNT.  One session with the unit path is
 * sgpr_seq_rows_above's score, one session with a path table is sgpr_seq_path_filter's.
 * - S, the session tables, sess / lo / hi, D_p(r, c) and Q_{p,sigma} are sgpr_session_filter's, bit for bit: the fp32
 *   additions in ascending d, the one multiplication by rcp[|D_p|], the context rows and the session window on the end
 *   point.
 * - MINIMUM TERM COUNT: min_terms lies in 1..L.  A candidate (p, sigma) takes part in the fold only when
 *   |D_p(r, c)| >= min_terms.  The fold is sgpr_seq_path_filter's - paths in ascending p within a direction, forward
 *   before reverse, q > best || best != best - run over the participating candidates in that order, the first of them
 *   initialising it; `code` is the winner's, direction bit | p << 1.  An end point with no participating candidate is
 *   NOT ELIGIBLE: never listed and never counted, not even at threshold = -inf.  With min_terms = 1 every candidate
 *   participates (d = 0 is always in D) and Q and code are sgpr_session_filter's bits.
 * - ELIGIBILITY: a pair (r, c) with ctx <= r < R is eligible when (1) it is not excluded by the session window
 *   (window >= 0, sess_col(c) == sess_col(self_r) and |c - self_r| <= window), (2) under SGPR_TOPK_CAUSAL, c < self_r,
 *   and (3) at least one candidate reaches min_terms; self_r = d_row_self[r] (device, [R]: context rows have entries
 *   too) or row0 + r.  A pair is selected when it is eligible and Q >= threshold.  A NaN Q never qualifies; a NaN
 *   threshold is SGPR_E_INVALID.
 * - OUTPUT: sgpr_seq_rows_above's exactly.  Row-major (r, then c ascending); d_rows holds r - ctx, d_values the bits of
 *   Q, d_codes (u8, may be NULL) the winner's code; d_row_ptr (int64 [R - ctx + 1], may be NULL) and *d_count are exact
 *   also when `capacity` cuts the output; capacity = 0 with NULL arrays counts only; two calls return identical bytes.
 *   ctx == R, R == 0 and M == 0 are valid empty calls.  A d_row_self entry outside [0, M) is reported by
 *   sgpr_check_status (the bit sgpr_rows_above raises).
 * - sgpr_session_rows_above: a resident matrix d_score [R][ld].  Two passes of sgpr_session_filter's tile kernel with
 *   sgpr_seq_rows_above's range-select epilogue (session_above_kernel in sgpr_seq.hip): no Q or code block exists.
 *   Its workspace equals sgpr_seq_rows_above_workspace_bytes.
 * - sgpr_score_session_above: the rectangle d_pooled_rows [R] x d_pooled_cols [M], every handle: sgpr_score_seq_above's
 *   row blocks (L - 1 context rows, the f16-range question answered once per call, positions continuing on the device
 *   across blocks) with the row table shifted per block as sgpr_score_session_topk shifts it.  Its workspace equals
 *   sgpr_score_seq_above_workspace_bytes at equal R, M, ctx, L, flags: the paths' halo lives in LDS.
 * Arguments are checked before the device is touched: those of sgpr_score_session_topk (paths, tables, window below -1),
 * those of sgpr_score_seq_above, and min_terms outside 1..L give SGPR_E_INVALID with a message naming the fault (the
 * workspace answer is 0 for invalid arguments), a workspace below the query SGPR_E_WORKSPACE.  Results depend on the
 * arguments alone.  Asynchronous on `stream`. */
size_t sgpr_session_rows_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx);
int sgpr_session_rows_above(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx,
                            const int32_t* d_row_self, int row0, int window, int flags, int L, const int32_t* h_offsets,
                            int n_paths, const int32_t* h_row_starts, int n_row_sessions, const int32_t* h_col_starts,
                            int n_col_sessions, int min_terms, float threshold, int32_t* d_rows, int32_t* d_cols,
                            float* d_values, unsigned char* d_codes, int64_t capacity, int64_t* d_row_ptr,
                            unsigned long long* d_count, void* d_workspace, size_t workspace_bytes, void* stream);
size_t sgpr_score_session_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int n_paths, int flags,
                                                int n_row_sessions, int n_col_sessions);
int sgpr_score_session_above(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                             int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L,
                             const int32_t* h_offsets, int n_paths, const int32_t* h_row_starts, int n_row_sessions,
                             const int32_t* h_col_starts, int n_col_sessions, int min_terms, float threshold,
                             int32_t* d_rows, int32_t* d_cols, float* d_values, unsigned char* d_codes, int64_t capacity,
                             int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace, size_t workspace_bytes,
                             void* stream);

/* LDS bytes per workgroup the embed kernel uses for (N, k) on this handle; 0 if unsupported. */
size_t sgpr_embed_lds_bytes(const sgpr_handle* h, int N, int k);

/* ---- stand-alone forms of the reference's building blocks (SURVEY.md 8b "signatures to keep") -------------------
 * Inside sgpr_embed / sgpr_forward_dense these run fused and never materialise their outputs; the entry points below
 * serve callers of the individual symbols.  They need no handle: a stand-alone module owns its own parameters, which
 * are passed as device pointers.  Sizes are checked first; an empty batch (B = 0) is a valid call that touches nothing,
 * and its pointers may be NULL (the data pointer of an empty torch tensor).
 *
 * sgpr_knn replaces dgcnn.knn (dgcnn.py:14-20): d_x [B,C,N] f32 -> d_idx [B,N,k] int64 (torch.topk's index type), the
 * k nearest candidates of every node under pd[i][j] = -|x_j|^2 + 2 x_i.x_j - |x_i|^2, best first; equal distances keep
 * the lower candidate index first (torch.topk's tie order is implementation-defined).  N <= SGPR_ANY_MAX_NODES, k <= N,
 * k <= SGPR_ANY_MAX_K, any C (beyond SGPR_MAX_NODES / SGPR_MAX_K, or when the graph does not fit one workgroup's LDS:
 * one wave per row instead of the LDS-resident kernel - the same keys and order, so the same lists).  A NaN distance
 * (a NaN node) or -inf one (an overflowing node) ranks after every finite distance, NaN last; every row still holds
 * k distinct indices. */
int sgpr_knn(const float* d_x, int B, int C, int N, int k, int64_t* d_idx, void* stream);

/* Replaces dgcnn.get_graph_feature (dgcnn.py:23-49) for given neighbour lists d_idx [B,N,k] (int64, from sgpr_knn or
 * the caller): d_out [B,2C,N,k] f32 = cat(x_j - x_i, x_i) in the reference's channel order (dgcnn.py:47).  An index
 * outside [0, N) is clamped to it (a negative one reads node 0, one >= N node N-1): no read leaves the graph. */
int sgpr_graph_feature(const float* d_x, const int64_t* d_idx, int B, int C, int N, int k, float* d_out, void* stream);

/* Replaces AttentionModule.forward (layers_batch.py:28-39): d_weight [F3,F3] (attention.weight_matrix),
 * d_emb [B,N,F3] -> d_rep [B,F3] (the graph-level representation) and d_att [B,N] (sigmoid scores; may be NULL).
 * No padding mask, divisor N - exactly like the reference.  F3 = 32. */
int sgpr_attention_pool(const float* d_weight, const float* d_emb, int B, int N, float* d_rep, float* d_att,
                        void* stream);

/* The same module at any width F <= SGPR_ANY_MAX_FILTERS_3 (d_weight [F,F], d_emb [B,N,F], d_rep [B,F]); plain fp32. */
int sgpr_attention_pool_any(const float* d_weight, const float* d_emb, int B, int N, int F, float* d_rep, float* d_att,
                            void* stream);

/* Replaces TenorNetworkModule.forward (layers_batch.py:70-83): d_weight [F3,F3,T], d_weight_block [T,2*F3],
 * d_bias [T], d_e1 / d_e2 [B,F3] -> d_out [B,T] = relu(e1^T W e2 + Wb [e1;e2] + bias).  F3 = 32, T = 16.
 * A NaN in e1 or e2 of a pair is NaN in all T outputs of that pair (the ReLU keeps a NaN); sgpr_ntn_any alike. */
int sgpr_ntn(const float* d_weight, const float* d_weight_block, const float* d_bias, const float* d_e1,
             const float* d_e2, int64_t B, float* d_out, void* stream);

/* The same module at any width F <= SGPR_ANY_MAX_FILTERS_3, T <= SGPR_ANY_MAX_NEURONS tensor neurons (d_weight [F,F,T],
 * d_weight_block [T,2F], d_bias [T], d_e1 / d_e2 [B,F] -> d_out [B,T]); plain fp32. */
int sgpr_ntn_any(const float* d_weight, const float* d_weight_block, const float* d_bias, const float* d_e1,
                 const float* d_e2, int64_t B, int F, int T, float* d_out, void* stream);

/* ---- geometric verification of loop-closure candidates --------------------------------------------
 * Planar consensus between the labelled centres of two graphs: is the pair one place, and what is the closure edge.
 * The reference has no such stage.  Pair p verifies row graph d_idx_a[p] of d_centers_a [GA,N,3] / d_labels_a [GA,N]
 * against column graph d_idx_b[p] of d_centers_b / d_labels_b [GB,...] - the packed arrays sgpr_embed reads, sensor frame
 * x forward, y left, z up; a slot with label < 0 is padding.  Every float32 operation below is rounded on its own (no
 * fused multiply-add; division and sqrt correctly rounded), so a record is reproducible bit for bit.
 *   hypothesis  h = (i, i', j, j'), i < i' real slots of A, j != j' real slots of B, la[i] == lb[j], la[i'] == lb[j'];
 *               u = a[i'].xy - a[i].xy, v = b[j'].xy - b[j].xy, lu = sqrt(ux ux + uy uy), lv alike; admissible iff
 *               lu >= min_base, lu lv > 0 (the float32 product den below: neither length is zero and the product does not
 *               underflow, so c and s are never 0 / 0) and |lu - lv| <= tau_edge
 *   coarse      den = lu lv, c = (ux vx + uy vy) / den, s = (ux vy - uy vx) / den, ma = 0.5 (a[i].xy + a[i'].xy), mb
 *               alike, tx = mb.x - (c ma.x - s ma.y), ty = mb.y - (s ma.x + c ma.y)
 *   inlier      node p of A with some q of B: la[p] == lb[q], |a[p].z - b[q].z| <= tau_z and, px = (c a[p].x - s a[p].y)
 *               + tx, py = (s a[p].x + c a[p].y) + ty, dx = px - b[q].x, dy = py - b[q].y: dx dx + dy dy <= tau_in tau_in
 *               (that product formed once in float32)
 *   best        the admissible hypothesis with the most inliers, ties to the lowest (i, i', j, j'): independent of the
 *               evaluation order
 *   cap         base pairs (i, i') ascend lexicographically; before one is started, max_hyp admissible hypotheses already
 *               evaluated stop the enumeration with SGPR_VERIFY_TRUNCATED; `hypotheses` = the number evaluated
 *   refined     one least-squares step in float64 (every operation rounded on its own, sums sequential over the inliers
 *               p ascending) on the matches q(p) = the qualifying q with the smallest dx dx + dy dy, ties to the lowest
 *               q: ca, cb the means, D = sum(ax~ bx~ + ay~ by~), X = sum(ax~ by~ - ay~ bx~) over the centred
 *               coordinates, nrm = sqrt(D D + X X), c = D / nrm, s = X / nrm, tx = cb.x - (c ca.x - s ca.y), ty = cb.y -
 *               (s ca.x + c ca.y); fewer than 2 inliers or nrm == 0: the coarse transform widened.  rmse = sqrt(sum r^2 /
 *               n) over the matches under it (NaN without a match); inliers_refined = the inlier count under the refined
 *               transform rounded to float32.
 * Flags: SGPR_VERIFY_NO_HYPOTHESIS (none admissible) and SGPR_VERIFY_NONFINITE (a real node of either graph has a NaN
 * or infinite coordinate; the pair is not evaluated) leave inliers 0, base -1, hypotheses 0 and NaN transforms / rmse;
 * an index outside its graph set, negative included (the -1 padding of a top-k list), gives an all-zero record with
 * SGPR_VERIFY_INVALID_INDEX and touches nothing else.  Every byte of every record is written; results depend on the
 * arguments alone.  With finite coordinates whose differences, squares and sums stay inside float32, flags == 0 comes
 * with a finite coarse and refined transform.  Finite coordinates beyond that (|x| of about 1e19 and more) pass the
 * input check and are evaluated by the same arithmetic: lu or lv may be +inf (|inf - inf| is NaN: inadmissible; a finite
 * length beside +inf is admissible only at tau_edge = +inf, with den = +inf and c = s = +-0 or NaN), so a record with
 * flags == 0 may then carry a transform that is no rotation or is NaN.  Callers keep coordinates in sensor range.
 * Checked before the device is touched: a NULL pointer (P > 0), P < 0, GA or GB < 0, a negative or NaN tolerance or
 * max_hyp < 1 give SGPR_E_INVALID, N outside 1..SGPR_VERIFY_MAX_NODES SGPR_E_NODES; P == 0 succeeds without a launch.  One workgroup per pair, no workspace, no atomics on global memory; work per pair is about
 * hypotheses x same-label correspondences, and a single base pair adds at most nB^2 hypotheses past the cap.
 * Handle-free; runs on the caller's current device, asynchronous on `stream`. */
typedef struct sgpr_verify_result {   /* 88 bytes */
    int32_t inliers, inliers_refined;
    int32_t base[4];                  /* i, i', j, j' (slot indices) */
    uint32_t hypotheses, flags;
    float coarse[4];                  /* c, s, tx, ty */
    double refined[4];
    double rmse;
} sgpr_verify_result;
#define SGPR_VERIFY_MAX_NODES 256
#define SGPR_VERIFY_INVALID_INDEX 1
#define SGPR_VERIFY_NO_HYPOTHESIS 2
#define SGPR_VERIFY_TRUNCATED 4
#define SGPR_VERIFY_NONFINITE 8
int sgpr_verify_pairs(const float* d_centers_a, const int32_t* d_labels_a, int GA,
                      const float* d_centers_b, const int32_t* d_labels_b, int GB, int N,
                      const int32_t* d_idx_a, const int32_t* d_idx_b, int64_t P,
                      float tau_edge, float tau_in, float tau_z, float min_base, int max_hyp,
                      sgpr_verify_result* d_out, void* stream);

/* ---- pairwise-consistent loop closures ---------------------------------------------------------------
 * Which of C verified closures agree with one another through the odometry of the drives, and a large set that agrees
 * pair by pair.  The reference has no such stage.  An SE(2) element E = (c, s, x, y) acts as p -> R p + t with
 * R = [[c, -s], [s, c]]; all arithmetic is float64 and every operation is rounded on its own (no fused multiply-add;
 * sqrt correctly rounded), so every output is reproducible bit for bit.
 *   compose(A, B) (B first): c = A.c B.c - A.s B.s, s = A.s B.c + A.c B.s, x = (A.c B.x - A.s B.y) + A.x,
 *               y = (A.s B.x + A.c B.y) + A.y;  inverse(A): c = A.c, s = -A.s, x = -(A.c A.x + A.s A.y),
 *               y = A.s A.x - A.c A.y
 *   closure p   d_rows[p], d_cols[p]: scan indices into d_Xr [MR,4] / d_Xc [MC,4], the planar odometry (each pose maps a
 *               point of that scan into its session's own frame; sessions may live in unrelated frames); d_T [C,4]: the
 *               `refined` field of sgpr_verify_pairs (a point of the row scan into the column scan); d_group[p]: the
 *               problem the closure belongs to (row session x column session).  Rp = Xr[rows[p]], Cp = Xc[cols[p]],
 *               G_p = compose(compose(Cp, T_p), inverse(Rp)), H_p = compose(inverse(T_p), inverse(Cp))
 *   void        rows[p] or cols[p] outside its table, group[p] outside [0, n_groups), or any of the 12 doubles read is
 *               not finite: a zero row and column, degree 0
 *   pair        p < q of one group, neither void: D = compose(compose(H_q, G_p), R_q), dx = R_q.x - R_p.x,
 *               dy = R_q.y - R_p.y, lever = sqrt(dx dx + dy dy), tau = max_trans + lever_gain lever; consistent iff
 *               D.c >= min_cos and D.x D.x + D.y D.y <= tau tau.  min_cos is a cosine, formed by the caller.
 *   d_adj       uint64 [C][ceil(C/64)]: bit q & 63 of word q >> 6 of row p = the test on (min(p,q), max(p,q)) - symmetric
 *               by construction; 0 on the diagonal, across groups and at bit positions >= C.  Every word is written.
 *   d_degree    int32 [C] = popcount of row p.
 *   workspace   sgpr_closure_consistency_workspace_bytes(C) = roundup(4 C, 256) + 96 C bytes, any contents.  After the
 *               call its first C int32 hold the members: group[p] of every closure that is not void, -1 of a void one -
 *               the d_group to hand to sgpr_consistent_set.
 * sgpr_consistent_set: the greedy clique of every group g on ANY bit matrix of that layout (symmetric or not).  cand =
 * the closures with d_group[p] == g; while cand is not empty: d(v) = popcount(row_v & cand & ~bit v) for every v in cand,
 * v* = the largest d, ties to the lowest index, d_rank[v*] = the number chosen before it in g, cand &= row_v* & ~bit v*.
 * Bits at or beyond C and diagonal bits are ignored, so the loop ends after at most |group| rounds whatever the matrix
 * holds.  d_rank int32 [C] (-1: not selected, d_group[p] outside [0, n_groups) included), d_group_size int32 [n_groups] =
 * the size of each clique.  Workspace: sgpr_consistent_set_workspace_bytes(C) = roundup(4 C, 256) bytes, any contents.
 * One workgroup per group; it keeps the counts up to date from what leaves cand (the same integers as recounting):
 * n ceil(C/64) word operations to start, then per round (candidates left) x (words in which cand lost a bit) - about
 * n^2 / 2 in all for a complete group of n closures - and three barriers per round.
 * Checked before the device is touched, each with a message naming the fault (and the workspace queries answer 0): a
 * NULL pointer with C > 0, C < 0 or > SGPR_CONSISTENCY_MAX_CLOSURES, MR or MC < 0, n_groups outside
 * 1..SGPR_CONSISTENCY_MAX_GROUPS, a negative or NaN max_trans or lever_gain, a NaN min_cos: SGPR_E_INVALID; a missing or
 * short workspace: SGPR_E_WORKSPACE.  C == 0 succeeds without a launch (d_group_size, if given, is zeroed).  Every
 * output byte is written; no atomics on global memory; results depend on the arguments alone.  Handle-free; both run on
 * the caller's current device, asynchronous on `stream`. */
#define SGPR_CONSISTENCY_MAX_CLOSURES 16384
#define SGPR_CONSISTENCY_MAX_GROUPS 4096
size_t sgpr_closure_consistency_workspace_bytes(int C);
int sgpr_closure_consistency(const int32_t* d_rows, const int32_t* d_cols, const double* d_T, int C, const double* d_Xr,
                             int MR, const double* d_Xc, int MC, const int32_t* d_group, int n_groups, double max_trans,
                             double min_cos, double lever_gain, uint64_t* d_adj, int32_t* d_degree, void* d_workspace,
                             size_t workspace_bytes, void* stream);
size_t sgpr_consistent_set_workspace_bytes(int C);
int sgpr_consistent_set(const uint64_t* d_adj, int C, const int32_t* d_group, int n_groups, int32_t* d_rank,
                        int32_t* d_group_size, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- training: one EdgeConv block with BatchNorm in train mode ---------------------------
 * Replaces, for training, get_graph_feature -> Conv2d 1x1 -> BatchNorm2d (batch statistics) -> LeakyReLU(0.2) -> max
 * over k (sg_net.py:50-73, 79-110; dgcnn.py:23-49) without forming the [B, 2C, N, k] edge tensor.  The caller splits
 * the conv weight W [F, 2C] = [Wa | Wb] and forms the per-node products d_P = Wa x and d_Q = (Wb - Wa) x, both
 * [B, F, N] f32, so that edge (i, k) with neighbour j = d_idx[b][i][k] has z = P[b,f,j] + Q[b,f,i].
 *   forward : d_y [B,F,N] = max_k LeakyReLU(gamma (z - mean) / sqrt(var + eps) + beta) with mean / biased var over all
 *             M = B N k edges per channel (d_mean, d_var [F]); saves d_sel [B,F,N] u8 (the selected k: the largest P
 *             for gamma >= 0, the smallest for gamma < 0, ties to the lowest k) and d_s1 [B,F,N] (sum_k P_nbr) for the
 *             backward.
 *   backward: from d_dy [B,F,N] and what the forward saved -> d_dP, d_dQ [B,F,N], d_dgamma, d_dbeta [F].  d_dQ also
 *             serves as the call's scratch (it may alias nothing else).
 * d_idx [B,N,k] int64 (sgpr_knn's lists); an index outside [0, N) is clamped to it.  N <= SGPR_TRAIN_MAX_NODES,
 * 1 <= k <= min(N, SGPR_TRAIN_MAX_K), any F >= 1, B >= 1.  d_workspace: sgpr_edgeconv_train_workspace_bytes(B, F)
 * bytes (per-graph fp64 partial sums), any contents.  Deterministic: no float atomics, fixed summation orders - two
 * calls on the same inputs give the same bits on any stream.  Handle-free; runs on the caller's current device. */
#define SGPR_TRAIN_MAX_NODES 1024
#define SGPR_TRAIN_MAX_K 64
size_t sgpr_edgeconv_train_workspace_bytes(int B, int F);
int sgpr_edgeconv_train_forward(const float* d_P, const float* d_Q, const int64_t* d_idx, const float* d_gamma,
                                const float* d_beta, int B, int F, int N, int k, float eps, float* d_y,
                                uint8_t* d_sel, float* d_s1, float* d_mean, float* d_var, void* d_workspace,
                                size_t workspace_bytes, void* stream);
int sgpr_edgeconv_train_backward(const float* d_dy, const float* d_P, const float* d_Q, const int64_t* d_idx,
                                 const uint8_t* d_sel, const float* d_s1, const float* d_mean, const float* d_var,
                                 const float* d_gamma, const float* d_beta, int B, int F, int N, int k, float eps,
                                 float* d_dP, float* d_dQ, float* d_dgamma, float* d_dbeta, void* d_workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- training: the tail over every ordered pair of a batch (tensor network + head + weighted BCE) ------------------
 * Replaces, for training, TenorNetworkModule.forward + fully_connected_first + scoring_layer + binary_cross_entropy
 * (layers_batch.py:70-83, sg_net.py:128-137) for ALL G x G ordered pairs of d_rep [G,F] at once, forward and backward,
 * without a [G^2, F, T] intermediate.  For the ordered pair (i, j):
 *   z_t = relu(sum_{f,g} rep[i,f] W[f,g,t] rep[j,g] + sum_f V[t,f] rep[i,f] + sum_g V[t,F+g] rep[j,g] + b_t),
 *   h = relu(fc1_w z + fc1_b), d_pred[i,j] = sigmoid(fc2_w . h + fc2_b) for every (i, j), the diagonal included.
 *   d_cls [G,G] u8: 0 = negative (y = 0, weight w_neg), 1 = positive (y = 1, weight w_pos), anything else = not in the
 *   loss; about ORDERED pairs, need not be symmetric.  d_loss[0] = sum w l / sum w with l = -(y log s + (1-y) log(1-s)),
 *   both logs clamped at -100; d_wsum[0] = sum w.  No labelled pair (or sum w = 0): loss 0 and every gradient 0.
 *   backward: d_dloss[0] (device) is the gradient at the loss; dlogit = (w / wsum) dloss (s - y) / max(s (1-s), 1e-12)
 *   * s (1-s) (torch's BCE-then-sigmoid chain: a saturated prediction has a zero gradient); ReLU' is 0 at 0.  Needs the
 *   forward's d_pred and d_wsum and the same inputs -> d_drep [G,F], d_dW [F,F,T], d_dV [T,2F], d_db [T], d_dfc1_w
 *   [H,T], d_dfc1_b [H], d_dfc2_w [H], d_dfc2_b [1].
 * fp32 operands, fp64 accumulators for every sum over pairs; no atomics and fixed summation orders, so two calls on the
 * same inputs give the same bits on any stream.  1 <= G <= SGPR_TRAIN_PAIRS_MAX_GRAPHS, F <= SGPR_ANY_MAX_FILTERS_3,
 * T, H <= SGPR_ANY_MAX_NEURONS (beyond: SGPR_E_DIMS, and the workspace query answers 0); a NULL pointer or a negative
 * weight is SGPR_E_INVALID, a missing or short workspace SGPR_E_WORKSPACE; all checked before the device is touched.
 * d_workspace: sgpr_pairs_train_workspace_bytes bytes, any contents.  Handle-free; runs on the caller's current device.
 * Non-finite inputs are handed on as torch's tail does, never swallowed: a NaN in d_rep[i] makes row i and column i of
 * d_pred NaN (every other entry keeps its bits), a NaN parameter makes d_pred NaN; if a NaN d_pred entry is labelled
 * (cls 0 / 1) the loss is NaN and every one of the eight gradients holds a non-finite value; if all of its pairs are
 * unlabelled the loss is unaffected, while d_rep, d_W, d_V, d_fc1_w and d_fc2_w still pick the NaN up (0 x NaN). */
#define SGPR_TRAIN_PAIRS_MAX_GRAPHS 1024
size_t sgpr_pairs_train_workspace_bytes(int G, int F, int T, int H);
int sgpr_pairs_train_forward(const float* d_rep, const float* d_W, const float* d_V, const float* d_b,
                             const float* d_fc1_w, const float* d_fc1_b, const float* d_fc2_w, const float* d_fc2_b,
                             const uint8_t* d_cls, float w_neg, float w_pos, int G, int F, int T, int H, float* d_pred,
                             float* d_loss, float* d_wsum, void* d_workspace, size_t workspace_bytes, void* stream);
int sgpr_pairs_train_backward(const float* d_dloss, const float* d_wsum, const float* d_pred, const float* d_rep,
                              const float* d_W, const float* d_V, const float* d_b, const float* d_fc1_w,
                              const float* d_fc1_b, const float* d_fc2_w, const float* d_fc2_b, const uint8_t* d_cls,
                              float w_neg, float w_pos, int G, int F, int T, int H, float* d_drep, float* d_dW,
                              float* d_dV, float* d_db, float* d_dfc1_w, float* d_dfc1_b, float* d_dfc2_w,
                              float* d_dfc2_b, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- upstream of the path: labelled LiDAR scan -> semantic-graph nodes -------------------------
 * Replaces, for one scan, gen_labels + the node half of gen_graphs (data_process/gen_label_graph.py:196-365):
 * raw SemanticKITTI labels are remapped (learning_map, :23-58); road / parking and the discarded classes produce no
 * node; a class that carries instance ids is grouped by instance (groups of <= 20 points dropped, :274); every other
 * class is clustered like PCL's EuclideanClusterExtraction (connected components of "squared distance < tolerance^2",
 * tolerance 0.2 / 0.5 / 2 m and minimum size 50..300 by class, maximum 50 000, :283-305); each surviving cluster whose
 * class is in node_map (:64-77) becomes a node: label = node_map[class], centre = mean of its points.
 *   d_points  [P, point_stride] f32 (x, y, z first; point_stride >= 3, 4 for KITTI .bin scans)
 *   d_labels  [P] u32 = semantic id | instance id << 16 (the .label file format)
 *   outputs   d_centers [max_nodes,3] f64, d_node_labels / d_node_sizes [max_nodes] i32, in the reference's node order
 *             (class ascending; instance id ascending / cluster size descending, lowest point index first among equal
 *             sizes - PCL leaves that last order unspecified); d_point_node [P] i32 = node of each point or -1 (may be
 *             NULL); d_num_nodes [1] i32 = number of nodes found (may exceed max_nodes: then only the first max_nodes are
 *             written; -1 if more than 8192 clusters qualified).
 * Non-finite coordinates: an axis of a node's centre is NaN iff some point of its cluster has a NaN or an infinity on
 * that axis; the other axes are the mean over all its points, as for a finite cluster.  Only a (class, instance) group
 * can hold such a point: under Euclidean clustering a point with a non-finite coordinate is in range of nothing, a
 * cluster of one below every minimum size, so its d_point_node is -1 and the nodes around it are unchanged (as are
 * road / parking, which never form nodes).  The remission column (index 3) is never read.
 * Limits: coordinates within +-110 km (|x| * 2^24 must stay far below 2^63); at most 32 768 distinct (class, instance
 * id) pairs in one scan - the pair table has 65 536 slots and its insertion does not terminate once the table is full.
 * Results do not depend on execution order (integer fixed-point centroid sums, lowest-index roots).  Handle-free; runs
 * on the caller's current device. */
size_t sgpr_cluster_workspace_bytes(int P);
int sgpr_cluster_scan(const float* d_points, int point_stride, const uint32_t* d_labels, int P, int max_nodes,
                      double* d_centers, int32_t* d_node_labels, int32_t* d_node_sizes, int32_t* d_point_node,
                      int32_t* d_num_nodes, void* d_workspace, size_t workspace_bytes, void* stream);

/* The edge rule of gen_graphs (gen_label_graph.py:367-385) for the n nodes of sgpr_cluster_scan: d_min_dis [n,n] f64 =
 * for i != j the distance between the point of cluster i and the point of cluster j that lie nearest to the midpoint of
 * the two centres (0 on the diagonal; NaN off the diagonal in the row and column of a node that has a NaN centre or
 * that no point of d_point_node carries - NaN <= 5 is false, so such a node gets no edge); the caller keeps the
 * pairs i < j with distance <= 5 m as edges of weight 1 - d/5.  The scorer never reads edges (utils.py:21-38 loads
 * nodes, centers and pose only); this serves writers of the reference's graph JSON.  d_workspace: n*n*4 bytes. */
int sgpr_graph_edges(const float* d_points, int point_stride, const int32_t* d_point_node, int P, int n,
                     const double* d_centers, double* d_min_dis, void* d_workspace, size_t workspace_bytes, void* stream);

/* Debug (per handle; not thread-safe; never set in production): a device array of 16 uint64 counters makes
 * sgpr_embed* run its profiling instance and add the
 * shader cycles wave 0 of every workgroup spends in each phase, barrier to barrier (0 stage, 1 select, 2 Gram,
 * 3 GEMM, 5 gather-max, 6 conv_end, 7 attention; 8..13 = sub-phases of the selection in sgpr_embed_debug with mask
 * bit 7).  The timers perturb the kernel (~1.6x); use the ablation mask for magnitudes.  NULL (default) disables. */
void sgpr_debug_set_profile_buffer(sgpr_handle* h, void* d_counters);

/* Debug / ablation timing only (results become invalid): bit 0 skips the kNN selection, bit 1 the per-node GEMMs,
 * bit 2 the Gram phase, bit 3 the gather-max; bit 4 returns right after dispatch, bit 5 after the input fetch;
 * bit 8 = nothing skipped (just selects the profiling instance); bits 9/10/11 keep the GEMM phase but drop its weight
 * loads / its MFMAs / its inner barrier; bit 12 runs the generic first semantic layer instead of the label lookup (valid
 * results); bit 13 forces the wide-range instance and bit 20 makes the producers of the split launch's odd slots
 * withhold their flag, so that their graphs reach the second pass through the late-producer path (both: valid
 * results, production kernels).  0 (default) = normal. */
void sgpr_debug_set_skip_mask(sgpr_handle* h, int mask);

/* 1: the handle's weights run on the default datapath (two f16 planes per matrix operand); 0: the checkpoint's folded
 * weights (or the super-node tables made from them) leave the f16 range, and every launch uses the wide-range
 * instance (three bf16 planes / fp32 rows).  Decided once, at sgpr_create.  (Weights BELOW f16's normal range keep an
 * absolute 2^-25 in the planes: harmless - the shipped checkpoints hold whole channels of 1e-30 .. 1e-7 behind dead
 * BatchNorm scales.) */
int sgpr_debug_uses_f16_planes(const sgpr_handle* h);

const char* sgpr_last_error(void);
int sgpr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_H */

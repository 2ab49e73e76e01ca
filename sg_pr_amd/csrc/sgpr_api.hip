// C-ABI entry points of libsgpr_hip.so (declared in include/sgpr.h).  The host-side weight preparation (eval-mode
// BatchNorm folding + kernel-ready layouts) is sgpr_model.hpp; sgpr_create uploads what it packs.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "sgpr_internal.hpp"
#include "sgpr_map.hpp"

namespace sgpr {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int raise_lds_limit(LdsLimitOnce* once, const void* kernel, int bytes, const char* what) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (dev < 64 && (once->done.load(std::memory_order_acquire) & bit)) return SGPR_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        int have = 0;
        (void)hipDeviceGetAttribute(&have, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        set_error(std::string(what) + ": the kernel needs " + std::to_string(bytes) + " bytes of LDS per workgroup, device " +
                  std::to_string(dev) + " offers " + std::to_string(have) + " (" + hipGetErrorString(e) + ")");
        return SGPR_E_HIP;
    }
    if (dev < 64) once->done.fetch_or(bit, std::memory_order_release);
    return SGPR_OK;
}

int hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return SGPR_E_HIP;
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, what);
}

// the caller's workspace holds the `need` bytes entry point fn asks for (need 0: any pointer, NULL included)
static bool workspace_ok(const char* fn, size_t need, const void* ws, size_t ws_bytes) {
    if (need > 0 && (!ws || ws_bytes < need)) {
        set_error(std::string(fn) + ": workspace of " + std::to_string(need) + " bytes required");
        return false;
    }
    return true;
}

// global row indices row0 .. row0 + R fit an int
static bool row0_ok(const char* fn, int row0, int R) {
    if ((int64_t)row0 + R > 0x7fffffffLL) {
        set_error(std::string(fn) + ": row0 + R must fit an int");
        return false;
    }
    return true;
}

}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_weights_count(const sgpr_dims* dims) { return dims ? weights_count(dims) : 0; }

int sgpr_abi_version(void) { return SGPR_ABI_VERSION; }

const char* sgpr_last_error(void) { return g_last_error.c_str(); }

// Every layout is packed on the host first (sgpr_model.hpp); what follows only uploads the buffers and turns their
// offsets into pointers.  A half-built handle is owned by `owner`: every failure path frees it through sgpr_destroy.
int sgpr_create(const float* weights, size_t n_floats, const sgpr_dims* dims, int device, sgpr_handle** out) {
    if (!weights || !dims || !out) {
        set_error("sgpr_create: NULL argument");
        return SGPR_E_INVALID;
    }
    if (!dims_supported(dims) && !dims_generic(dims)) {
        set_error("sgpr_create: architecture outside what the any-shape kernels serve (labels <= 64, filters <= 256, "
                  "filters_3 <= 128, tensor / bottleneck neurons <= 64)");
        return SGPR_E_DIMS;
    }
    if (n_floats != weights_count(dims)) {
        set_error("sgpr_create: weights blob has " + std::to_string(n_floats) + " floats, expected " +
                  std::to_string(weights_count(dims)));
        return SGPR_E_BLOB;
    }
    // larger than the shape the tuned kernels are built for {labels 12, filters 64/64/32, tensor 16, bottleneck 16}:
    // the handle runs every call on the any-shape kernels (sgpr_generic.hip); else the any-shape model of the same
    // checkpoint serves node_num / K beyond the tuned kernels' limits
    const bool generic_only = !dims_supported(dims);
    const FoldedNet net = fold_model(weights, dims);
    const PackedBuilt pb = generic_only ? PackedBuilt() : pack_built(net);
    const PackedGeneric pg = pack_generic(net);
    const PackedWide pw = pack_wide(net, generic_only);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (device < 0 || device >= ndev) {
        set_error("sgpr_create: device " + std::to_string(device) + " of " + std::to_string(ndev));
        return SGPR_E_INVALID;
    }
    DeviceGuard guard(device);   // the caller's current device is restored on return
    struct Destroy {
        void operator()(sgpr_handle* p) const { sgpr_destroy(p); }
    };
    std::unique_ptr<sgpr_handle, Destroy> owner(new sgpr_handle());
    sgpr_handle* h = owner.get();
    memset(static_cast<void*>(h), 0, sizeof(*h));
    h->device = device;
    h->dims = *dims;             // (what the caller loaded; the tuned kernels run on the built shapes)
    h->generic_only = generic_only ? 1 : 0;
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->num_cus <= 0)
        h->num_cus = 256;

    auto upload = [&e](void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    e = hipMalloc(reinterpret_cast<void**>(&h->d_status), sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->d_status, 0, sizeof(int32_t));
    if (e == hipSuccess && !generic_only) e = hipMalloc(reinterpret_cast<void**>(&h->d_blob), pb.blob.size() * sizeof(float));
    if (!generic_only) upload(h->d_blob, pb.blob.data(), pb.blob.size() * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "sgpr_create: device allocation / upload");
    e = hipMalloc(reinterpret_cast<void**>(&h->d_gblob), pg.blob.size() * sizeof(float));
    upload(h->d_gblob, pg.blob.data(), pg.blob.size() * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "sgpr_create: any-shape model");
    if (pw.ok) {
        e = hipMalloc(&h->d_wblob, pw.plane_bytes + pw.tbs.size() * sizeof(float));
        upload(h->d_wblob, pw.planes.data(), pw.planes.size() * sizeof(unsigned short));
        upload(static_cast<char*>(h->d_wblob) + pw.plane_bytes, pw.tbs.data(), pw.tbs.size() * sizeof(float));
        if (e != hipSuccess) return hip_fail(e, "sgpr_create: matrix-core form of the any-shape model");
    }

    GenericModel& m = h->gm;
    m.L = dims->num_labels; m.f1 = dims->filters_1; m.f2 = dims->filters_2; m.f3 = dims->filters_3;
    m.T = dims->tensor_neurons; m.B = dims->bottle_neck_neurons;
    m.cmax = pg.cmax;
    const float* gv = h->d_gblob;
    for (int l = 0; l < 6; ++l) {
        m.cin[l] = pg.cin[l];
        m.cout[l] = pg.cout[l];
        m.wa[l] = gv + pg.off_wa[l];
        m.wb[l] = gv + pg.off_wb[l];
        m.tb[l] = gv + pg.off_tb[l];
    }
    m.w_end = gv + pg.off_wend;
    m.t_end = gv + pg.off_tend;
    m.att_w = gv + pg.off_tail[kAttW];
    m.ntn_w = gv + pg.off_tail[kNtnW];
    m.ntn_wb = gv + pg.off_tail[kNtnWb];
    m.ntn_bias = gv + pg.off_tail[kNtnBias];
    m.fc1_w = gv + pg.off_tail[kFc1W];
    m.fc1_b = gv + pg.off_tail[kFc1B];
    m.fc2_w = gv + pg.off_tail[kFc2W];
    m.fc2_b = gv + pg.off_tail[kFc2B];
    m.head_scale = pg.head.scale;
    m.head_nl2e = pg.head.nl2e;
    m.head_f16 = pg.head.f16_ok;

    if (pw.ok) {
        WideModel& wm = h->wm;
        const unsigned short* pv = static_cast<const unsigned short*>(h->d_wblob);
        const float* tv = reinterpret_cast<const float*>(static_cast<const char*>(h->d_wblob) + pw.plane_bytes);
        for (int l = 0; l < 6; ++l) {
            wm.cinP[l] = pw.cinP[l];
            wm.coutP[l] = pw.coutP[l];
            wm.wh[l] = pv + pw.off_wh[l];
            wm.tbp[l] = tv + pw.off_tbp[l];
        }
        wm.wh_end = pv + pw.off_wh[6];
        wm.tbp_end = tv + pw.off_tbp[6];
        wm.F3P = pw.F3P;
        wm.att_w = m.att_w;
        wm.L = m.L;
        wm.f3 = m.f3;
        wm.ok = 1;
    }
    if (generic_only) {
        *out = owner.release();
        return SGPR_OK;
    }

    h->blob_floats = pb.blob.size();
    DevWeights& w = h->w;
    for (int l = 0; l < 6; ++l) {
        w.wf[l] = h->d_blob + pb.off_wf[l];
        w.tb[l] = h->d_blob + pb.off_tb[l];
        w.wb[l] = reinterpret_cast<const unsigned short*>(h->d_blob + pb.off_wb[l]);
        w.wh[l] = reinterpret_cast<const unsigned short*>(h->d_blob + pb.off_wh[l]);
        w.kp[l] = pb.kp[l];
        w.cout[l] = pb.cout[l];
    }
    w.wf_end = h->d_blob + pb.off_wf[6];
    w.tb_end = h->d_blob + pb.off_tb[6];
    w.wb_end = reinterpret_cast<const unsigned short*>(h->d_blob + pb.off_wb[6]);
    w.wh_end = reinterpret_cast<const unsigned short*>(h->d_blob + pb.off_wh[6]);
    w.att_w = h->d_blob + pb.off_tail[kAttW];
    w.ntn_w = h->d_blob + pb.off_tail[kNtnW];
    w.ntn_wt = h->d_blob + pb.off_ntwt;
    w.ntn_wb = h->d_blob + pb.off_tail[kNtnWb];
    w.ntn_bias = h->d_blob + pb.off_tail[kNtnBias];
    w.fc1_w = h->d_blob + pb.off_tail[kFc1W];
    w.fc1_b = h->d_blob + pb.off_tail[kFc1B];
    w.fc2_w = h->d_blob + pb.off_tail[kFc2W];
    w.fc2_b = h->d_blob + pb.off_tail[kFc2B];
    w.head_scale = pb.head.scale;
    w.head_nl2e = pb.head.nl2e;
    h->head_f16 = pb.head.f16_ok;
    h->f16_weights = pb.f16_ok ? 1 : 0;
    if (pb.f16_ok) {
        // the graph-independent part of the super-node branch, by the kernels' own instructions (bit-identical to the
        // per-graph path); skipped when a layer-1 output leaves the f16 range (the per-graph path then flags the graph)
        float* tab = h->d_blob + pb.off_semtab;
        float vmax = INFINITY;
        const int rc = launch_sem_tables(w, tab, tab + kSemTableFloats, nullptr);
        if (rc != SGPR_OK) return rc;
        e = hipMemcpy(&vmax, tab + kSemTableFloats, sizeof(float), hipMemcpyDeviceToHost);   // (synchronises)
        if (e != hipSuccess) return hip_fail(e, "sgpr_create: super-node tables");
        if (vmax < 60000.f) {
            w.sem_g = tab;
            w.sem_xx = tab + 4 * 256;
            w.sem_a2 = w.sem_xx + 32;
            w.sem_b2 = w.sem_a2 + 2 * 16 * 64;
        }
    }
    *out = owner.release();
    return SGPR_OK;
}

void sgpr_destroy(sgpr_handle* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    if (h->d_gblob) (void)hipFree(h->d_gblob);
    if (h->d_wblob) (void)hipFree(h->d_wblob);
    if (h->d_blob) (void)hipFree(h->d_blob);
    if (h->d_status) (void)hipFree(h->d_status);
    delete h;
}

#ifndef SGPR_SPLIT_SEM
#define SGPR_SPLIT_SEM 1     // lean production launches on packed input hand the semantic branch to semantic waves
#endif

// wide: use the wide-range X layouts (bf16 planes / fp32 rows) instead of the default f16 planes
// debug-mask bits that keep the production kernel instance: 8192 forces the wide-range instance, 1 << 20 makes the split
// launch's odd producers withhold their flag (test hook for the late-producer hand-over to the second pass)
static constexpr int kProductionSkipBits = 8192 | (1 << 20);
#ifndef SGPR_AUTO_LEAN
#define SGPR_AUTO_LEAN 1      // 0 (A/B builds): a launch without a node_cap promise is sized for node_num
#endif
static bool wide_range(const sgpr_handle* h) { return !h->f16_weights || (h->dbg_skip & 8192); }
// the tails of the built shape at fp32's range: a wide-range handle, or a scoring head whose fold leaves the f16 range
// (head_range: the embed keeps its f16 planes then)
static bool tail_wide(const sgpr_handle* h) { return wide_range(h) || !h->head_f16; }

static int check_nk(int G, int N, int k, int node_cap, EmbedPlan* plan, bool wide, bool small_park = false) {
    if (G < 0) {
        set_error("negative graph count");
        return SGPR_E_INVALID;
    }
    if (N < 1 || N > SGPR_MAX_NODES) {
        set_error("node_num " + std::to_string(N) + " outside [1, " + std::to_string(SGPR_MAX_NODES) + "]");
        return SGPR_E_NODES;
    }
    if (k < 1 || k > SGPR_MAX_K || k > N) {
        set_error("K " + std::to_string(k) + " outside [1, min(node_num, " + std::to_string(SGPR_MAX_K) + ")]");
        return SGPR_E_K;
    }
    if (node_cap < 0) {
        set_error("negative node_cap");
        return SGPR_E_INVALID;
    }
    if (!make_embed_plan(N, node_cap, k, plan, wide, small_park)) {
        set_error("no LDS plan for node_num " + std::to_string(N) + ", K " + std::to_string(k));
        return SGPR_E_NODES;
    }
    return SGPR_OK;
}

// workspace of an embed launch over G graphs of N slots:  redo flags [G] (one byte per launch slot, written by the f16
// instance, read by the wide-range second pass) | parked first-branch output [G][round16(N)][32] f32 when N > 128
// (sized for the uncapped plan: the second pass never uses a node_cap)
// (+ one word at the end of the flag region: EmbedArgs::redo_count)
static size_t embed_flag_bytes(int G) { return ((size_t)G + 8 + 255) & ~(size_t)255; }
static unsigned* embed_redo_count(unsigned char* flags, int G) {
    return reinterpret_cast<unsigned*>(flags + embed_flag_bytes(G) - 8);
}
static size_t embed_park_bytes(int G, int N) {
    return ((N > 128 ? (size_t)G * ((N + 15) / 16 * 16) * 32 * sizeof(float) : 0) + 255) & ~(size_t)255;
}
// ... | split launch (sgpr_internal.hpp, EmbedArgs::sem_tab): one 64-bit flag (the flag array rounded up to 16 bytes: the
// rows behind it are read and written as float4) + 16 rows of 32 floats per launch slot; a split launch has at most
// num_cus / 2 graphs (launch_embed), so the region is sized for that many slots, not for G
// The split launch serves at most min(num_cus / 2, kMaxSplitGraphs) graphs: launch_embed needs a CU per workgroup of
// both halves, and the workspace region is sized for kMaxSplitGraphs slots whatever the device (workspace queries work
// without a device: MI355X's 256 CUs / 2).  On a part with more CUs, launches of 129 .. num_cus / 2 graphs run unsplit
// (same results; the latency form simply stops at 128 graphs).
constexpr int kMaxSplitGraphs = 128;
static int embed_sem_slots(const sgpr_handle*, int G) { return G < kMaxSplitGraphs ? G : kMaxSplitGraphs; }
static size_t embed_sem_flag_bytes(int slots) { return ((size_t)slots * sizeof(unsigned long long) + 15) & ~(size_t)15; }
static size_t embed_sem_bytes(const sgpr_handle* h, int G) {
    const int slots = embed_sem_slots(h, G);
    return embed_sem_flag_bytes(slots) + (size_t)slots * 16 * 32 * sizeof(float);
}
static size_t embed_ws_bytes(const sgpr_handle* h, int G, int N) {
    return embed_flag_bytes(G) + embed_park_bytes(G, N) + embed_sem_bytes(h, G);
}

// which launches run on the any-shape kernels (sgpr_generic.hip): every launch of a handle whose architecture is larger
// than the built shape, and launches beyond the tuned kernels' node_num / K limits on any handle
static bool needs_generic(const sgpr_handle* h, int N, int k) {
    return h->generic_only || N > SGPR_MAX_NODES || k > SGPR_MAX_K;
}
static bool generic_nk_ok(int N, int k) {
    return N >= 1 && N <= SGPR_GENERIC_MAX_NODES && k >= 1 && k <= SGPR_GENERIC_MAX_K && k <= N;
}
static int pooled_width(const sgpr_handle* h) { return h->generic_only ? h->gm.f3 : kF3; }

// the matrix-core any-shape embed (sgpr_wide.hip) flags the graphs it hands to the plain-fp32 kernel: one byte per launch slot
// ahead of that kernel's scratch area
static size_t wide_flag_bytes(const sgpr_handle* h, int G, int N, int k) {
    return (h->generic_only && h->wm.ok && k == 10 && N <= SGPR_WIDE_MAX_NODES) ? (((size_t)G + 8 + 255) & ~(size_t)255) : 0;   // (+ the token word)
}

size_t sgpr_embed_workspace_bytes(const sgpr_handle* h, int G, int N, int k) {
    EmbedPlan p;
    if (!h || G < 0) return 0;
    if (needs_generic(h, N, k))
        return generic_nk_ok(N, k) ? generic_embed_ws_bytes(h, G, N, k) + wide_flag_bytes(h, G, N, k) + 256 : 0;
    if (!make_embed_plan(N, 0, k, &p)) return 0;
    return embed_ws_bytes(h, G, N);
}

size_t sgpr_embed_lds_bytes(const sgpr_handle* h, int N, int k) {
    EmbedPlan p;
    if (!h) return 0;
    if (needs_generic(h, N, k)) return generic_nk_ok(N, k) ? generic_embed_lds_bytes(h, N, k) : 0;
    if (!make_embed_plan(N, 0, k, &p)) return 0;
    return (size_t)p.lds_bytes;
}

int sgpr_pooled_width(const sgpr_handle* h) { return h ? pooled_width(h) : 0; }
int sgpr_is_any_shape(const sgpr_handle* h) { return (h && h->generic_only) ? 1 : 0; }

// an embed launch on the any-shape kernels
static int embed_generic(const sgpr_handle* h, EmbedArgs a, int N, int k, void* ws, size_t ws_bytes, void* stream) {
    if ((a.dbg_layers || a.dbg_knn) && h->generic_only) {
        set_error("sgpr_embed_debug: the layer dump's rows are 64 floats - not served for an architecture beyond the built shape");
        return SGPR_E_DIMS;
    }
    if (a.G < 0) {
        set_error("negative graph count");
        return SGPR_E_INVALID;
    }
    if (N < 1 || N > SGPR_GENERIC_MAX_NODES) {
        set_error("node_num " + std::to_string(N) + " outside [1, " + std::to_string(SGPR_GENERIC_MAX_NODES) + "]");
        return SGPR_E_NODES;
    }
    if (k < 1 || k > SGPR_GENERIC_MAX_K || k > N) {
        set_error("K " + std::to_string(k) + " outside [1, min(node_num, " + std::to_string(SGPR_GENERIC_MAX_K) + ")]");
        return SGPR_E_K;
    }
    const size_t flags = wide_flag_bytes(h, a.G, N, k);
    const size_t need = generic_embed_ws_bytes(h, a.G, N, k) + flags;
    if (need > 0 && (!ws || ws_bytes < need)) {
        set_error("sgpr_embed: workspace of " + std::to_string(need) + " bytes required (sgpr_embed_workspace_bytes)");
        return SGPR_E_WORKSPACE;
    }
    a.status = h->d_status;
    a.num_labels = h->dims.num_labels;
    a.skip = h->dbg_skip;                // (bits 24..27: ablation of the any-shape kernel's phases, tools/run_anyshape.py)
    DeviceGuard guard(h->device);
    // a moderately larger architecture (labels <= 32, filters <= 128 / 128 / 64) at node_num <= 112, K = 10: the matrix-core
    // embed; the plain-fp32 kernel then takes only the graphs it flagged (values outside the f16 range)
    if (flags > 0 && wide_embed_serves(h, a, N, k)) {
        a.redo = static_cast<unsigned char*>(ws);
        a.redo_count = reinterpret_cast<unsigned*>(a.redo + flags - 8);
        {
            // this call's token: a counter spread over 32 bits (a fresh workspace holds stale small integers - labels, flags,
            // earlier counters - which a bare counter meets by chance; a match costs the pass a scan of the flags, never a result)
            static std::atomic<unsigned> epoch{0u};
            unsigned e = (++epoch) * 0x9E3779B1u;
            if (e == 0u) e = 0x9E3779B1u;
            a.sem_epoch = e;
        }
        const int rc = launch_embed_wide(h, a, N, k, static_cast<hipStream_t>(stream));
        if (rc != SGPR_OK) return rc;
        a.auto_over = 7;
    }
    return launch_embed_generic(h, a, N, k, static_cast<unsigned char*>(ws) + flags, static_cast<hipStream_t>(stream));
}

static int embed_common(const sgpr_handle* h, EmbedArgs a, int N, int k, int node_cap, void* ws, size_t ws_bytes,
                        void* stream, int total_graphs = -1) {   // total_graphs: G when a.ids lists a subset
    if (h && a.G == 0) return SGPR_OK;
    if (!h || !a.pooled || (!a.dense && (!a.centers || (!a.labels && !(a.rag_off && a.rag_lab))))) {
        set_error("sgpr_embed: NULL argument");
        return SGPR_E_INVALID;
    }
    if (needs_generic(h, N, k)) return embed_generic(h, a, N, k, ws, ws_bytes, stream);
    // with at most one graph per CU there is nothing to overlap: keep the 512-thread workgroups (lower latency)
    a.promise = (node_cap > 0 && node_cap < N) ? node_cap : N;   // still enforced (a broken promise stays loud)
    const bool promised = node_cap > 0 && node_cap < N;
    if (a.G <= h->num_cus) node_cap = 0;
    EmbedPlan plan;
    // production launches (no dumps, timers or ablation) of lean plans park only the super-node rows
    const bool production = !a.dbg_layers && !a.dbg_knn && !h->dbg_prof && !(h->dbg_skip & ~kProductionSkipBits);
    // No promise, more graphs than CUs (the throughput regime): the launch still runs on the lean 64-row plan - four
    // workgroups per CU, what KITTI-like data fits into - and a graph with more processed slots is handed to the
    // owned-rows instance sized for node_num in the same call (launch_embed), instead of every graph paying for the
    // largest one could be.  (The reference has no such prerequisite either: sg_net.py:503-525.)
    // A promise of 65 .. kTwoTierCap slots (K <= 16) takes the same two tiers: the graphs of up to 64 slots on the lean plan,
    // the others on the owned-rows instance sized for the PROMISED cap - a mixed data set no longer pays every graph at the
    // size of its largest; the promise stays enforced (a graph beyond it: NaN + SGPR_E_NODES).  Measured (tools/run_auto.py,
    // ordered launches, 4541 graphs of node_num 100): 25..70 nodes (cap 71, 15 % above 64 slots) 322 -> 207 us, 40..85
    // nodes (cap 86, 48 %) 352 -> 334; but 2048 graphs of 20..120 nodes in 256 slots (cap 121, 56 % above 64 and most of the
    // work in them) 153 -> 188: two launches that each under-fill the device.  The library sees the cap, not the data: the
    // two tiers stop at a cap of 96 (six row tiles), where an oversize graph costs little more than a lean one.
    constexpr int kTwoTierCap = 96;
    bool auto_lean = false;
    const int over_cap = promised ? node_cap : N;
    if ((!promised || (node_cap > 64 && node_cap <= kTwoTierCap)) && production && !wide_range(h) && a.G > h->num_cus && N > 64 &&
        SGPR_AUTO_LEAN) {
        EmbedPlan lean;
        if (make_embed_plan(N, 64, k, &lean, false, true) && lean.lean) {
            node_cap = 64;
            auto_lean = true;
        }
    }
    int rc = check_nk(a.G, N, k, node_cap, &plan, wide_range(h), production);
    if (rc != SGPR_OK) return rc;
    // graphs are addressed by their own index: an ordered launch needs rows for all of them
    const int gtot = total_graphs < 0 ? a.G : total_graphs;
    const size_t need = embed_ws_bytes(h, gtot, N);
    if (!ws || ws_bytes < need) {
        set_error("sgpr_embed: workspace of " + std::to_string(need) + " bytes required (sgpr_embed_workspace_bytes)");
        return SGPR_E_WORKSPACE;
    }
    a.redo = static_cast<unsigned char*>(ws);
    a.redo_count = embed_redo_count(a.redo, gtot);
    a.over_count = a.redo_count + 1;                 // (the second word of the 8 bytes behind the flags)
    a.auto_over = auto_lean ? 1 : 0;
    a.over_cap = over_cap;
    a.park_ws = reinterpret_cast<float*>(static_cast<unsigned char*>(ws) + embed_flag_bytes(gtot));
    unsigned char* sem = static_cast<unsigned char*>(ws) + embed_flag_bytes(gtot) + embed_park_bytes(gtot, N);
    a.sem_flag = reinterpret_cast<unsigned long long*>(sem);               // indexed by launch slot (< a.G <= num_cus / 2)
    a.sem_tab = reinterpret_cast<float*>(sem + embed_sem_flag_bytes(embed_sem_slots(h, gtot)));
    if (a.G > kMaxSplitGraphs) a.sem_tab = nullptr;                        // (no split launch: the region holds fewer than G slots)
#if !SGPR_SPLIT_SEM
    a.sem_tab = nullptr;                                                   // (A/B builds: the unsplit launch)
#endif
    a.status = h->d_status;
    a.prof = h->dbg_prof;
    a.skip = h->dbg_skip;
    a.num_labels = h->dims.num_labels;
    DeviceGuard guard(h->device);
    return launch_embed(h, plan, a, static_cast<hipStream_t>(stream));
}

int sgpr_embed(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int k,
               float* d_pooled, float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes,
               void* stream) {
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.centers = d_centers;
    a.labels = d_labels;
    a.G = G;
    a.pooled = d_pooled;
    a.att = d_att;
    a.emb = d_emb;
    return embed_common(h, a, N, k, 0, d_workspace, workspace_bytes, stream);
}

int sgpr_embed_capped(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int node_cap,
                      int k, float* d_pooled, float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes,
                      void* stream) {
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.centers = d_centers;
    a.labels = d_labels;
    a.G = G;
    a.pooled = d_pooled;
    a.att = d_att;
    a.emb = d_emb;
    return embed_common(h, a, N, k, node_cap, d_workspace, workspace_bytes, stream);
}

int sgpr_embed_ordered(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int node_cap,
                       int k, const int32_t* d_order, int n_order, float* d_pooled, float* d_att, float* d_emb,
                       void* d_workspace, size_t workspace_bytes, void* stream) {
    if (G < 0 || n_order < 0 || n_order > G || (n_order > 0 && !d_order)) {
        set_error("sgpr_embed_ordered: order list of " + std::to_string(n_order) + " entries for " + std::to_string(G) +
                  " graphs");
        return SGPR_E_INVALID;
    }
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.centers = d_centers;
    a.labels = d_labels;
    a.ids = d_order;
    a.G = n_order;
    a.pooled = d_pooled;
    a.att = d_att;
    a.emb = d_emb;
    return embed_common(h, a, N, k, node_cap, d_workspace, workspace_bytes, stream, G);
}

size_t sgpr_size_order_workspace_bytes(int G) { return G < 0 ? 0 : size_order_ws_bytes(G); }

int sgpr_size_order(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, const int64_t* d_offsets, int G,
                    int N, int k, int32_t* d_order, int32_t* d_info, void* d_workspace, size_t workspace_bytes,
                    void* stream) {
    if (!h || G < 0 || !d_info || (G > 0 && (!d_order || (!d_offsets && (!d_centers || !d_labels))))) {
        set_error("sgpr_size_order: NULL argument or negative count");
        return SGPR_E_INVALID;
    }
    if (N < 1 || N > SGPR_MAX_NODES || k < 1 || k > N) {
        set_error("sgpr_size_order: node_num " + std::to_string(N) + " / K " + std::to_string(k) +
                  " outside the tuned kernels' range (the any-shape kernels take no node_cap)");
        return SGPR_E_NODES;
    }
    if (!d_workspace || workspace_bytes < size_order_ws_bytes(G)) {
        set_error("sgpr_size_order: workspace of " + std::to_string(size_order_ws_bytes(G)) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    DeviceGuard guard(h->device);
    return launch_size_order(d_centers, d_labels, reinterpret_cast<const long long*>(d_offsets), G, N, k, h->dims.num_labels,
                             d_order, d_info, d_workspace, static_cast<hipStream_t>(stream));
}

int sgpr_embed_ragged(const sgpr_handle* h, const float* d_centers, const int8_t* d_labels, const int64_t* d_offsets,
                      int G, int N, int node_cap, int k, const int32_t* d_order, int n_order, float* d_pooled,
                      float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (G < 0 || n_order < 0 || n_order > G || (n_order > 0 && !d_order) || (G > 0 && !d_offsets)) {
        set_error("sgpr_embed_ragged: order list of " + std::to_string(n_order) + " entries for " + std::to_string(G) +
                  " graphs, or no offsets");
        return SGPR_E_INVALID;
    }
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.centers = d_centers;
    a.rag_lab = reinterpret_cast<const signed char*>(d_labels);
    a.rag_off = reinterpret_cast<const long long*>(d_offsets);
    a.ids = d_order;
    a.G = d_order ? n_order : G;
    a.pooled = d_pooled;
    a.att = d_att;
    a.emb = d_emb;
    return embed_common(h, a, N, k, node_cap, d_workspace, workspace_bytes, stream, G);
}

int sgpr_embed_dense(const sgpr_handle* h, const float* d_features, int G, int N, int k, float* d_pooled,
                     float* d_att, float* d_emb, void* d_workspace, size_t workspace_bytes, void* stream) {
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.dense = d_features;
    a.G = G;
    a.pooled = d_pooled;
    a.att = d_att;
    a.emb = d_emb;
    return embed_common(h, a, N, k, 0, d_workspace, workspace_bytes, stream);
}

int sgpr_embed_debug(const sgpr_handle* h, const float* d_centers, const int32_t* d_labels, int G, int N, int k,
                     float* d_pooled, float* d_att, float* d_emb, float* d_layers, int32_t* d_knn,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.centers = d_centers;
    a.labels = d_labels;
    a.G = G;
    a.pooled = d_pooled;
    a.att = d_att;
    a.emb = d_emb;
    a.dbg_layers = d_layers;
    a.dbg_knn = d_knn;
    return embed_common(h, a, N, k, 0, d_workspace, workspace_bytes, stream);
}

int sgpr_score_pairs(const sgpr_handle* h, const float* d_pooled1, const int32_t* d_idx1, const float* d_pooled2,
                     const int32_t* d_idx2, int64_t P, float* d_score, void* stream) {
    if (!h || !d_pooled1 || !d_pooled2 || !d_score || P < 0) {
        set_error("sgpr_score_pairs: NULL argument or negative count");
        return SGPR_E_INVALID;
    }
    DeviceGuard guard(h->device);
    if (h->generic_only)
        return launch_score_generic(h, d_pooled1, d_idx1, d_pooled2, d_idx2, P, 0, d_score, 0, static_cast<hipStream_t>(stream));
    return launch_score_pairs(h, d_pooled1, d_idx1, d_pooled2, d_idx2, P, d_score, static_cast<hipStream_t>(stream));
}

size_t sgpr_pair_plan_ints(int64_t P, int R) {
    if (P < 0 || R < 0) return 0;
    const int64_t rows = P < R ? P : R;                       // distinct row graphs at most
    const int64_t items = P / 16 + rows;                      // sum over rows of ceil(count / 16) at most
    return (size_t)(rows + items + (items + 1) + 2 * P);
}

int sgpr_pair_plan(const int32_t* h_idx1, const int32_t* h_idx2, int64_t P, int R, int M, int32_t* h_plan,
                   size_t plan_capacity_ints, size_t* plan_ints, int32_t* n_rows, int32_t* n_items) {
    if (P < 0 || P >= 0x7fffffffLL || R < 0 || M < 0 || (P > 0 && (!h_idx1 || !h_idx2)) || !plan_ints || !n_rows || !n_items) {
        set_error("sgpr_pair_plan: NULL argument, negative count or 2^31 pairs or more");
        return SGPR_E_INVALID;
    }
    // (host allocations proportional to R: a failure is an error code, never an exception across the C boundary)
    std::vector<int32_t> count, cursor;
    try {
        count.assign((size_t)R + 1, 0);
        cursor.assign((size_t)R + 1, 0);
    } catch (const std::exception&) {
        set_error("sgpr_pair_plan: out of host memory for " + std::to_string(R) + " row graphs");
        return SGPR_E_INVALID;
    }
    for (int64_t p = 0; p < P; ++p) {
        const int32_t a = h_idx1[p], b = h_idx2[p];
        if (a < 0 || a >= R || b < 0 || b >= M) {
            set_error("sgpr_pair_plan: pair " + std::to_string(p) + " = (" + std::to_string(a) + ", " + std::to_string(b) +
                      ") outside [0, " + std::to_string(R) + ") x [0, " + std::to_string(M) + ")");
            return SGPR_E_INVALID;
        }
        ++count[a];
    }
    int64_t nr = 0, ni = 0;
    for (int r = 0; r < R; ++r)
        if (count[r]) {
            ++nr;
            ni += (count[r] + 15) / 16;
        }
    const size_t need = (size_t)(nr + ni + (ni + 1) + 2 * P);
    *plan_ints = need;
    *n_rows = (int32_t)nr;
    *n_items = (int32_t)ni;
    if (!h_plan || plan_capacity_ints < need) {
        if (!h_plan && plan_capacity_ints == 0) return SGPR_OK;           // size query
        set_error("sgpr_pair_plan: plan needs " + std::to_string(need) + " int32 words");
        return SGPR_E_WORKSPACE;
    }
    int32_t* row_ids = h_plan;
    int32_t* item_row = row_ids + nr;
    int32_t* item_beg = item_row + ni;
    int32_t* cols = item_beg + ni + 1;
    int32_t* pos = cols + P;
    int32_t at = 0, cr = 0, it = 0;
    for (int r = 0; r < R; ++r) {
        cursor[r] = at;
        if (!count[r]) continue;
        row_ids[cr] = r;
        for (int32_t c0 = 0; c0 < count[r]; c0 += 16) {
            item_row[it] = cr;
            item_beg[it++] = at + c0;
        }
        at += count[r];
        ++cr;
    }
    item_beg[it] = (int32_t)P;
    for (int64_t p = 0; p < P; ++p) {
        const int32_t w = cursor[h_idx1[p]]++;
        cols[w] = h_idx2[p];
        pos[w] = (int32_t)p;
    }
    return SGPR_OK;
}

size_t sgpr_score_pair_list_workspace_bytes(const sgpr_handle* h, int n_rows, int M) {
    if (!h || n_rows < 0 || M < 0) return 0;
    return score_pair_list_ws_bytes(n_rows, M);
}

int sgpr_score_pair_list(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         const int32_t* d_plan, int n_rows, int n_items, int64_t P, float* d_score, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
    if (!h || R < 0 || M < 0 || P < 0 || P >= 0x7fffffffLL || n_rows < 0 || n_rows > R || n_items < 0 ||
        (P > 0 && (!d_pooled_rows || !d_pooled_cols || !d_plan || !d_score || n_rows == 0 || n_items == 0 || n_items > P))) {
        set_error("sgpr_score_pair_list: NULL argument, negative count or a plan that does not fit (P, R)");
        return SGPR_E_INVALID;
    }
    if (P == 0) return SGPR_OK;
    if (h->generic_only) {                                   // (an architecture beyond the built shape: the plan walked on the
        DeviceGuard guard(h->device);                        //  any-shape tail, pair by pair - the bits of sgpr_score_pairs; no workspace)
        return launch_score_plan_generic(h, d_pooled_rows, d_pooled_cols, d_plan, n_rows, n_items, P, d_score,
                                         static_cast<hipStream_t>(stream));
    }
    if (!workspace_ok("sgpr_score_pair_list", score_pair_list_ws_bytes(n_rows, M), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    // (a wide-range tail: the kernel's exact fp32 per-pair arithmetic - the f16 planes are not this handle's, and there is
    //  no three-plane instance of the list kernel)
    return launch_score_pair_list(h, d_pooled_rows, d_pooled_cols, M, d_plan, n_rows, n_items, P, d_score, d_workspace,
                                  static_cast<hipStream_t>(stream), tail_wide(h));
}

size_t sgpr_score_all_pairs_workspace_bytes(const sgpr_handle* h, int R, int M) {
    if (!h || R < 0 || M < 0) return 0;
    if (h->generic_only && h->wm.ok) return std::max(score_all_pairs_ws_bytes(R, M), wide_tail_ws_bytes(R, M));
    return score_all_pairs_ws_bytes(R, M);
}

// One rectangle of an any-shape handle: a moderately larger tensor network (pooled width <= 64, <= 32 neurons) on the matrix
// cores (sgpr_wide.hip) when the caller brought its workspace; the plain-fp32 kernel behind it runs only if the inputs left
// the f16 range (a device word).  Handles beyond those limits: the plain-fp32 kernel alone, no workspace.
// fresh = false: the range header at the start of ws already holds a larger rectangle's (score_row_blocks).
static int score_rect_any_shape(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, float* score, int64_t ld,
                                void* ws, size_t ws_bytes, hipStream_t stream, bool fresh = true) {
    const unsigned* gate = nullptr;
    if (wide_tail_serves(h) && ws && ws_bytes >= wide_tail_ws_bytes(R, M)) {
        const int rc = launch_score_all_pairs_wide_any(h, rows, R, cols, M, score, ld, ws, &gate, stream, fresh);
        if (rc != SGPR_OK) return rc;
    }
    return launch_score_generic(h, rows, nullptr, cols, nullptr, (int64_t)R * M, M, score, ld, stream, gate);
}

int sgpr_score_all_pairs(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         float* d_score, int64_t ld, void* d_workspace, size_t workspace_bytes, void* stream) {
    // an empty rectangle (a rank whose row shard is empty: fewer graphs than ranks) needs no buffers at all
    if (!h || R < 0 || M < 0 || ld < M || (R > 0 && M > 0 && (!d_pooled_rows || !d_pooled_cols || !d_score))) {
        set_error("sgpr_score_all_pairs: NULL argument, negative count or ld < M");
        return SGPR_E_INVALID;
    }
    if (R == 0 || M == 0) return SGPR_OK;
    if (h->generic_only) {
        DeviceGuard guard(h->device);
        return score_rect_any_shape(h, d_pooled_rows, R, d_pooled_cols, M, d_score, ld, d_workspace, workspace_bytes,
                                    static_cast<hipStream_t>(stream));
    }
    if (!workspace_ok("sgpr_score_all_pairs", score_all_pairs_ws_bytes(R, M), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    // (debug bit 13 / weights or head outside the f16 range: the instance with three bf16 planes per operand, as for the embed)
    return launch_score_all_pairs(h, d_pooled_rows, R, d_pooled_cols, M, d_score, ld, d_workspace,
                                  static_cast<hipStream_t>(stream), tail_wide(h));
}

static int check_jobs(const sgpr_handle* h, int n, const sgpr_pairs_job* jobs) {
    if (!h || n < 0 || n > SGPR_MAX_PAIR_JOBS || (n > 0 && !jobs)) {
        set_error("sgpr_score_all_pairs_multi: NULL argument or not 0.." + std::to_string(SGPR_MAX_PAIR_JOBS) + " jobs");
        return SGPR_E_INVALID;
    }
    for (int j = 0; j < n; ++j) {
        const sgpr_pairs_job& q = jobs[j];
        if (q.R < 0 || q.M < 0 || q.ld < q.M ||
            (q.R > 0 && q.M > 0 && (!q.d_pooled_rows || !q.d_pooled_cols || !q.d_score))) {
            set_error("sgpr_score_all_pairs_multi: job " + std::to_string(j) + ": NULL pointer, negative count or ld < M");
            return SGPR_E_INVALID;
        }
    }
    return SGPR_OK;
}

// ---- the fused epilogues of the all-pairs tail (sgpr_score_topk, _mine, _above, _positives, _threshold_counts) run on
//      the production handle.  The other handles (wide-range, any-shape) score bounded row blocks with their own tail
//      and hand each block to the epilogue's matrix kernel (the same selection, bit-equal to matrix + selection).
static const size_t kScoreBlockBytes = (size_t)64 << 20;   // score block of the row-block path

static bool has_fused_epilogues(const sgpr_handle* h) { return !h->generic_only && !tail_wide(h); }

// rows scored per block; ctx_rows (sgpr_score_seq_topk): rows of the block that hold the block before's last scores
static int score_block_rows(int R, int M, int ctx_rows = 0) {
    const size_t rows = kScoreBlockBytes / ((size_t)M * sizeof(float));
    const size_t fresh = rows > (size_t)ctx_rows ? rows - ctx_rows : 0;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)R, fresh));
}

// row-block path layout: score block [ctx_rows + rb][M] | the caller's head (head_bytes) | the block's all-pairs workspace
static size_t row_blocks_ws_bytes(const sgpr_handle* h, int R, int M, size_t head_bytes, int ctx_rows = 0) {
    const int rb = score_block_rows(R, M, ctx_rows);
    return a256(((size_t)ctx_rows + rb) * M * sizeof(float)) + head_bytes + sgpr_score_all_pairs_workspace_bytes(h, rb, M);
}

// the caller's head of that layout (where the call's f16 range sits, if it has one)
static unsigned char* row_blocks_head(void* ws, int R, int M, int ctx_rows = 0) {
    const size_t rows = (size_t)ctx_rows + score_block_rows(R, M, ctx_rows);
    return static_cast<unsigned char*>(ws) + a256(rows * M * sizeof(float));
}

// sgpr_score_all_pairs on rows [r0, r0 + n) of the rectangle, one block after the other, each followed by
// consume(block, head, r0): block the n scored rows [n][M] (ld M), head the caller's region of the workspace.
// The f16-range question is the whole rectangle's, as in sgpr_score_all_pairs on it: on an any-shape handle's matrix-core
// tail a first pass preps every block into the all-pairs region, its TailHdr cleared once and accumulating the maxima of
// all blocks, and no block's scoring clears it (the other handles' row blocks take the three-plane instance: no gate).
// crng (a float4 in the caller's head, used on the production handle alone): there launch_call_range answers the
// question once for all blocks, and every block's all-pairs launch reads that answer instead of its own rows' partials.
// ctx_rows > 0 (sgpr_score_seq_topk): the block buffer has ctx_rows rows in front of the scored ones; after each block
// but the last, the last ctx_rows scored rows are copied there, so consume finds the min(ctx_rows, r0) rows before r0
// right in front of `block`.
extern "C++" {   // (a template, inside the C-ABI block)
template <class Consume>
static int score_row_blocks(const sgpr_handle* h, const PooledRect& p, size_t head_bytes, void* ws, size_t ws_bytes,
                            void* stream, Consume&& consume, float* crng = nullptr, int ctx_rows = 0) {
    const int R = p.R, M = p.M, rb = score_block_rows(R, M, ctx_rows), pw = pooled_width(h);
    const float *rows = p.rows, *cols = p.cols;
    float* carry = static_cast<float*>(ws);
    float* block = carry + (size_t)ctx_rows * M;
    unsigned char* head = row_blocks_head(ws, R, M, ctx_rows);
    unsigned char* aws = head + head_bytes;
    const size_t aws_bytes = ws_bytes - (size_t)(aws - static_cast<unsigned char*>(ws));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool one_range = h->generic_only && wide_tail_serves(h) && rb < R;
    const bool call_range = crng && has_fused_epilogues(h) && rb < R;
    if (call_range) {
        const int rc = launch_call_range(h, rows, R, cols, M, rb, aws, crng, s);
        if (rc != SGPR_OK) return rc;
    }
    if (one_range) {
        hipError_t e = hipMemsetAsync(aws, 0, 256, s);    // (the TailHdr)
        if (e != hipSuccess) return hip_fail(e, "row blocks: clearing the range header");
        for (int r0 = 0; r0 < R; r0 += rb) {
            const int rc = launch_wide_tail_prep(h, rows + (size_t)r0 * pw, std::min(rb, R - r0), cols, M, aws, s);
            if (rc != SGPR_OK) return rc;
        }
    }
    for (int r0 = 0; r0 < R; r0 += rb) {
        const int n = std::min(rb, R - r0);
        int rc = one_range  ? score_rect_any_shape(h, rows + (size_t)r0 * pw, n, cols, M, block, M, aws, aws_bytes, s, false)
                 : call_range ? launch_score_all_pairs(h, rows + (size_t)r0 * pw, n, cols, M, block, M, aws, s, false, crng)
                              : sgpr_score_all_pairs(h, rows + (size_t)r0 * pw, n, cols, M, block, M, aws, aws_bytes, stream);
        if (rc != SGPR_OK) return rc;
        const ScoreBlock scored = {block, n, M, M};
        rc = consume(scored, head, r0);
        if (rc != SGPR_OK) return rc;
        if (ctx_rows > 0 && r0 + n < R) {
            // rows [n, n + ctx_rows) of the buffer move to its front: one copy, or (a block shorter than the context:
            // the ranges overlap) ascending pieces of n rows, each disjoint from its source
            for (int i = 0; i < ctx_rows; i += n) {
                const int m = std::min(n, ctx_rows - i);
                hipError_t e = hipMemcpyAsync(carry + (size_t)i * M, carry + (size_t)(i + n) * M,
                                              (size_t)m * M * sizeof(float), hipMemcpyDeviceToDevice, s);
                if (e != hipSuccess) return hip_fail(e, "row blocks: carrying the context rows");
            }
        }
    }
    return SGPR_OK;
}
}  // extern "C++"

size_t sgpr_score_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > 16 || (flags & ~SGPR_TOPK_CAUSAL)) return 0;
    if (R == 0 || M == 0) return 0;
    if (has_fused_epilogues(h)) return score_topk_ws_bytes(h, R, M, k);
    return row_blocks_ws_bytes(h, R, M, 0);
}

int sgpr_score_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                    const int32_t* d_row_self, int row0, int window, int flags, int k, float* d_values, int32_t* d_indices,
                    void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!h || R < 0 || M < 0 || (R > 0 && (!d_values || !d_indices)) || (R > 0 && M > 0 && (!d_pooled_rows || !d_pooled_cols))) {
        set_error("sgpr_score_topk: NULL argument or negative count");
        return SGPR_E_INVALID;
    }
    if (k < 1 || k > 16) {
        set_error("sgpr_score_topk: k must lie in 1..16");
        return SGPR_E_INVALID;
    }
    if (flags & ~SGPR_TOPK_CAUSAL) {
        set_error("sgpr_score_topk: unknown flag bits " + std::to_string(flags & ~SGPR_TOPK_CAUSAL));
        return SGPR_E_INVALID;
    }
    if (!row0_ok("sgpr_score_topk", row0, R)) return SGPR_E_INVALID;
    if (!workspace_ok("sgpr_score_topk", sgpr_score_topk_workspace_bytes(h, R, M, k, flags), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == 0) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const Eligible elig = eligible(d_row_self, row0, window, flags);
    const ListOut out = {d_values, d_indices, k, nullptr};
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (M == 0 || has_fused_epilogues(h)) return launch_score_topk(h, rect, elig, out, d_workspace, s);
    auto select = [&](const ScoreBlock& block, unsigned char*, int r0) {
        return launch_topk_rows_ext(block, elig.from(r0), out.at(r0), h->d_status, s);
    };
    return score_row_blocks(h, rect, 0, d_workspace, workspace_bytes, stream, select);
}

// ---- sgpr_score_topk_large / sgpr_topk_rows_large: k up to SGPR_TOPK_LARGE_MAX through the large-k selection
//      (sgpr_select.hip); the pooled form scores 64 MB row blocks on every handle and selects from each
static bool topk_large_args_ok(const char* fn, int R, int k, int flags, int row0) {
    if (k < 1 || k > SGPR_TOPK_LARGE_MAX) {
        set_error(std::string(fn) + ": k must lie in 1.." + std::to_string(SGPR_TOPK_LARGE_MAX));
        return false;
    }
    if (flags & ~SGPR_TOPK_CAUSAL) {
        set_error(std::string(fn) + ": unknown flag bits " + std::to_string(flags & ~SGPR_TOPK_CAUSAL));
        return false;
    }
    return row0_ok(fn, row0, R);
}

// head of the pooled form: the call's f16 range (a float4) | the selection's workspace for one block
static size_t topk_large_head_bytes(int R, int M) { return 256 + a256(select_ws_bytes(score_block_rows(R, M), M)); }

size_t sgpr_topk_rows_large_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > SGPR_TOPK_LARGE_MAX || (flags & ~SGPR_TOPK_CAUSAL)) return 0;
    return select_ws_bytes(R, M);
}

int sgpr_topk_rows_large(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const int32_t* d_row_self,
                         int row0, int window, int flags, int k, float* d_values, int32_t* d_indices, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
    if (!h || (!d_score && M > 0) || !d_values || !d_indices || R < 0 || M < 0 || ld < M || window < -1) {
        set_error("sgpr_topk_rows_large: NULL argument, negative size, leading dimension below M or window below -1");
        return SGPR_E_INVALID;
    }
    if (!topk_large_args_ok("sgpr_topk_rows_large", R, k, flags, row0)) return SGPR_E_INVALID;
    if (!workspace_ok("sgpr_topk_rows_large", sgpr_topk_rows_large_workspace_bytes(h, R, M, k, flags), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == 0) return SGPR_OK;
    const ScoreBlock block = {d_score, R, M, ld};
    const ListOut out = {d_values, d_indices, k, nullptr};
    DeviceGuard guard(h->device);
    return launch_select_rows(block, eligible(d_row_self, row0, window, flags), out, d_workspace, false, h->d_status,
                              static_cast<hipStream_t>(stream));
}

size_t sgpr_score_topk_large_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > SGPR_TOPK_LARGE_MAX || (flags & ~SGPR_TOPK_CAUSAL)) return 0;
    if (R == 0 || M == 0) return 0;
    return row_blocks_ws_bytes(h, R, M, topk_large_head_bytes(R, M));
}

int sgpr_score_topk_large(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                          const int32_t* d_row_self, int row0, int window, int flags, int k, float* d_values,
                          int32_t* d_indices, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!h || R < 0 || M < 0 || (R > 0 && (!d_values || !d_indices)) || (R > 0 && M > 0 && (!d_pooled_rows || !d_pooled_cols))) {
        set_error("sgpr_score_topk_large: NULL argument or negative count");
        return SGPR_E_INVALID;
    }
    if (!topk_large_args_ok("sgpr_score_topk_large", R, k, flags, row0)) return SGPR_E_INVALID;
    if (!workspace_ok("sgpr_score_topk_large", sgpr_score_topk_large_workspace_bytes(h, R, M, k, flags), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == 0) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const Eligible elig = eligible(d_row_self, row0, window, flags);
    const ListOut out = {d_values, d_indices, k, nullptr};
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (M == 0) return launch_select_rows(ScoreBlock{nullptr, R, 0, 0}, elig, out, nullptr, false, h->d_status, s);
    float* crng = reinterpret_cast<float*>(row_blocks_head(d_workspace, R, M));
    auto select = [&](const ScoreBlock& block, unsigned char* head, int r0) {
        return launch_select_rows(block, elig.from(r0), out.at(r0), head + 256, r0 > 0, h->d_status, s);
    };
    return score_row_blocks(h, rect, topk_large_head_bytes(R, M), d_workspace, workspace_bytes, stream, select, crng);
}

// ---- sgpr_seq_filter / sgpr_score_seq_topk: the diagonal score filter (seq_filter_kernel; the family: sgpr_seq.hip) on a resident matrix, and on
//      row blocks that carry their last L - 1 rows over as the next block's context, each selected by the large-k selection
static const int kSeqFlags = SGPR_TOPK_CAUSAL | SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE;

static bool seq_args_ok(const char* fn, int R, int ctx, int L, int flags, int allowed) {
    if (L < 1 || L > SGPR_SEQ_MAX_LEN) {
        set_error(std::string(fn) + ": the sequence length must lie in 1.." + std::to_string(SGPR_SEQ_MAX_LEN));
        return false;
    }
    if (ctx < 0 || ctx > R) {
        set_error(std::string(fn) + ": ctx must lie in 0..R");
        return false;
    }
    if (flags & ~allowed) {
        set_error(std::string(fn) + ": unknown flag bits " + std::to_string(flags & ~allowed));
        return false;
    }
    if (!(flags & (SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE))) {
        set_error(std::string(fn) + ": no direction flag (SGPR_SEQ_FORWARD, SGPR_SEQ_REVERSE)");
        return false;
    }
    return true;
}

int sgpr_seq_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx, int L, int flags,
                    float* d_out, int64_t ldo, unsigned char* d_dir, void* stream) {
    if (!h || R < 0 || M < 0 || ld < M || ldo < M) {
        set_error("sgpr_seq_filter: NULL handle, negative size or leading dimension below M");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok("sgpr_seq_filter", R, ctx, L, flags, SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)) return SGPR_E_INVALID;
    if (R > ctx && M > 0 && (!d_score || !d_out)) {       // (an empty result needs no buffers)
        set_error("sgpr_seq_filter: NULL argument");
        return SGPR_E_INVALID;
    }
    if (R == ctx || M == 0) return SGPR_OK;
    const ScoreBlock block = {d_score, R, M, ld};
    const FilterOut out = {d_out, ldo, d_dir, ldo};
    DeviceGuard guard(h->device);
    return launch_seq_filter(block, seq_spec(ctx, L, flags), out, static_cast<hipStream_t>(stream));
}

static bool seq_both(int flags) { return (flags & SGPR_SEQ_FORWARD) && (flags & SGPR_SEQ_REVERSE); }

// ---- the ranking pipeline of sgpr_score_seq_topk, _peak_topk, _path_topk and _session_topk.  Row blocks that carry their
//      last L - 1 rows over as the next block's context, each going through: score block -> [diagonal / path / session
//      filter into a Q block] -> [peak filter into a P block] -> the large-k selection -> the directions / codes of the
//      selected columns.
enum RankFilter { kRankNone, kRankDiagonal, kRankPaths, kRankSessions };

struct RankStages {
    RankFilter filter;     // kRankNone: the ranked score is S itself (L = 1 before a peak step: S * rcp[1] is S)
    bool peak;             // the peak step runs: a P block sits in front of the Q block
    int radius;
    bool code_block;       // the filter writes a dir / code block behind the Q block
    bool code_room;        // the head has room for that block
    bool filter_window;    // the window is the filter's (sessions): the selection runs without one
};

static RankStages rank_stages(RankFilter filter, bool peak, int radius, bool code_block, bool code_room) {
    RankStages st;
    st.filter = filter;
    st.peak = peak;
    st.radius = radius;
    st.code_block = code_block;
    st.code_room = code_room;
    st.filter_window = false;
    return st;
}

// sgpr_score_seq_topk: the diagonal filter at every L; a dir block when both directions are asked for
static RankStages seq_stages(int flags) { return rank_stages(kRankDiagonal, false, 0, seq_both(flags), seq_both(flags)); }

// sgpr_score_peak_topk: the peak step at every radius, the diagonal filter when L > 1 (L = 1, both directions: the two
// sums are one number and forward wins the tie - direction 0, no dir block)
static RankStages peak_stages(int L, int radius, int flags) {
    const bool dir = L > 1 && seq_both(flags);
    return rank_stages(L > 1 ? kRankDiagonal : kRankNone, true, radius, dir, dir);
}

// sgpr_score_path_topk: the peak step only when radius > 0, the path filter unless L = 1 comes before a peak step (every
// candidate is S itself).  Codes: both directions or several paths; one direction and several paths keep their room
// in the head even where no filter runs
static RankStages path_stages(int L, int n_paths, int radius, int flags) {
    const bool filter = radius == 0 || L > 1;
    return rank_stages(filter ? kRankPaths : kRankNone, radius > 0, radius, filter && (seq_both(flags) || n_paths > 1),
                       seq_both(flags) ? filter : n_paths > 1);
}

// sgpr_score_session_topk: sgpr_score_path_topk's at radius 0 with the session filter, which applies the window itself
static RankStages session_stages(int L, int n_paths, int flags) {
    RankStages st = path_stages(L, std::max(n_paths, 1), 0, flags);
    st.filter = kRankSessions;
    st.filter_window = true;
    return st;
}

// the pipeline's head: the call's f16 range (a float4) | the selection's workspace for one block | [P block [rb][M]] |
// [Q block [rb][M]] | [dir / code block [rb][M] u8]
static size_t rank_head_bytes(int R, int M, int L, const RankStages& st) {
    const size_t rb = (size_t)score_block_rows(R, M, L - 1), blk = a256(rb * M * sizeof(float));
    return 256 + a256(select_ws_bytes((int)rb, M)) + (st.peak ? blk : 0) + (st.filter != kRankNone ? blk : 0) +
           (st.code_room ? a256(rb * M) : 0);
}

// what a row block with context means to the ranking, range and evaluation pipelines: the block scored rows r0 ..
// r0 + scored.R - 1 of the call, and min(L - 1, r0) rows of the block before sit right in front of them
struct BlockView {
    int first;         // the block's first output row (a row of the call)
    int no;            // its output rows; <= 0: context rows only
    int base;          // the call's row of the rectangle's row 0
    ScoreBlock rect;   // what a filter sees: from global row 0, or L - 1 rows back (no sum reaches further)
    BlockView(const ScoreBlock& scored, int r0, int ctx, int L) : rect(scored) {
        const int c = std::min(L - 1, r0);
        first = std::max(r0, ctx);
        no = r0 + scored.R - first;
        base = r0 - c;
        rect.score -= (size_t)c * scored.M;
        rect.R += c;
    }
};

// the call's SeqSpec as the rectangle of a block sees it (shift_row_table): the context is what lies in front of the
// first output row, and the row-session table moves with the rectangle (nullptr stays nullptr: one session).  A session
// that starts before `base` starts at the rectangle's row 0 - where it matters (base > 0) every output row has its L - 1
// rows inside the rectangle, and a depth of L is a depth of L from either start (so min_terms sees the same)
struct ShiftedSeq : SeqSpec {
    int32_t local[SGPR_SESSION_MAX];
    ShiftedSeq(const SeqSpec& seq, const BlockView& v) : SeqSpec(seq) {
        ctx = v.first - v.base;
        if (!row_starts) return;
        for (int j = 0; j < n_row; ++j)
            local[j] = (int32_t)std::min<int64_t>(std::max<int64_t>((int64_t)seq.row_starts[j] - v.base, 0), v.rect.R);
        row_starts = local;
    }
    ShiftedSeq(const ShiftedSeq&) = delete;
};

// arguments and workspace already checked, R > ctx.  Without a code block the listed code is the first direction asked
// for, path 0: one candidate, or L = 1 where all candidates are one number and the first one keeps a listed, hence
// non-NaN, entry (forward wins the tie)
static int rank_row_blocks(const sgpr_handle* h, const PooledRect& p, const SeqSpec& seq, const Eligible& elig,
                           const ListOut& out, const RankStages& st, void* d_workspace, size_t workspace_bytes,
                           void* stream) {
    const int R = p.R, M = p.M, ctx = seq.ctx, L = seq.L, fixed_code = (seq.dirs & SGPR_SEQ_FORWARD) ? 0 : 1;
    const Eligible sel = st.filter_window ? elig.without_window() : elig;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (M == 0) {
        const ScoreBlock none = {nullptr, R - ctx, 0, 0};
        const int rc = launch_select_rows(none, sel.from(ctx), out, nullptr, false, h->d_status, s);
        if (rc != SGPR_OK || !out.codes) return rc;
        return launch_seq_dirs(out.idx, R - ctx, out.k, nullptr, 0, fixed_code, out.codes, s);
    }
    const int rb = score_block_rows(R, M, L - 1);
    const size_t sel_bytes = a256(select_ws_bytes(rb, M)), blk_bytes = a256((size_t)rb * M * sizeof(float));
    const size_t p_at = 256 + sel_bytes, q_at = p_at + (st.peak ? blk_bytes : 0);
    float* crng = reinterpret_cast<float*>(row_blocks_head(d_workspace, R, M, L - 1));
    int clean_rows = 0;                                   // histogram rows the selection before left clear
    auto select = [&](const ScoreBlock& scored, unsigned char* head, int r0) {
        const BlockView v(scored, r0, ctx, L);
        if (v.no <= 0) return (int)SGPR_OK;               // context rows only
        const ShiftedSeq sq(seq, v);
        unsigned char* code = st.code_block ? head + q_at + blk_bytes : nullptr;
        const FilterOut q = {reinterpret_cast<float*>(head + q_at), M, code, M};
        int rc = SGPR_OK;
        if (st.filter == kRankDiagonal)
            rc = launch_seq_filter(v.rect, sq, q, s);
        else if (st.filter == kRankPaths)
            rc = launch_seq_path_filter(v.rect, sq, q, s);
        else if (st.filter == kRankSessions)              // row_self / row0 and the row table move with the rectangle
            rc = launch_session_filter(v.rect, sq, elig.from(v.base), q, s);
        if (rc != SGPR_OK) return rc;
        ScoreBlock x = {st.filter != kRankNone ? q.out : scored.score + (size_t)(v.first - r0) * M, v.no, M, M};
        if (st.peak) {                                    // (rows are independent: no context rows of its own)
            float* peaks = reinterpret_cast<float*>(head + p_at);
            rc = launch_peak_filter(x, elig.from(v.first), st.radius, peaks, M, s);
            if (rc != SGPR_OK) return rc;
            x.score = peaks;
        }
        const ListOut o = out.at(v.first - ctx);
        rc = launch_select_rows(x, sel.from(v.first), o, head + 256, select_group_rows(v.no) <= clean_rows, h->d_status, s);
        // (the first block's outputs start at ctx: the block after it may select more rows, whose histograms reach into
        //  what this one used for its state and counts)
        clean_rows = select_group_rows(v.no);
        if (rc != SGPR_OK || !o.codes) return rc;
        return launch_seq_dirs(o.idx, v.no, o.k, q.code, M, fixed_code, o.codes, s);
    };
    return score_row_blocks(h, p, rank_head_bytes(R, M, L, st), d_workspace, workspace_bytes, stream, select, crng, L - 1);
}

size_t sgpr_score_seq_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int k, int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > SGPR_TOPK_LARGE_MAX || L < 1 || L > SGPR_SEQ_MAX_LEN || ctx < 0 || ctx > R ||
        (flags & ~kSeqFlags) || !(flags & (SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)))
        return 0;
    if (R == ctx || M == 0) return 0;
    return row_blocks_ws_bytes(h, R, M, rank_head_bytes(R, M, L, seq_stages(flags)), L - 1);
}

int sgpr_score_seq_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                        int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L, int k,
                        float* d_values, int32_t* d_indices, unsigned char* d_dirs, void* d_workspace,
                        size_t workspace_bytes, void* stream) {
    if (!h || R < 0 || M < 0) {
        set_error("sgpr_score_seq_topk: NULL handle or negative count");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok("sgpr_score_seq_topk", R, ctx, L, flags, kSeqFlags)) return SGPR_E_INVALID;
    if ((R > ctx && (!d_values || !d_indices)) || (R > ctx && M > 0 && (!d_pooled_rows || !d_pooled_cols))) {
        set_error("sgpr_score_seq_topk: NULL argument");
        return SGPR_E_INVALID;
    }
    if (!topk_large_args_ok("sgpr_score_seq_topk", R, k, flags & SGPR_TOPK_CAUSAL, row0)) return SGPR_E_INVALID;
    if (!workspace_ok("sgpr_score_seq_topk", sgpr_score_seq_topk_workspace_bytes(h, R, M, ctx, L, k, flags), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == ctx) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const ListOut out = {d_values, d_indices, k, d_dirs};
    return rank_row_blocks(h, rect, seq_spec(ctx, L, flags), eligible(d_row_self, row0, window, flags), out,
                           seq_stages(flags), d_workspace, workspace_bytes, stream);
}

// ---- sgpr_peak_filter / sgpr_score_peak_topk: per-row score peaks within a scan radius (sgpr_peak.hip) on a resident
//      block, and on sgpr_score_seq_topk's row blocks: score, diagonal filter (L > 1), peak filter into a P block, the
//      large-k selection on P.  Rows are independent, so the peak step needs no context rows of its own
static bool peak_radius_ok(const char* fn, int radius) {
    if (radius < 0 || radius > SGPR_PEAK_MAX_RADIUS) {
        set_error(std::string(fn) + ": the radius must lie in 0.." + std::to_string(SGPR_PEAK_MAX_RADIUS));
        return false;
    }
    return true;
}

int sgpr_peak_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const int32_t* d_row_self,
                     int row0, int window, int flags, int radius, float* d_out, int64_t ldo, void* stream) {
    if (!h || R < 0 || M < 0 || ld < M || ldo < M || window < -1) {
        set_error("sgpr_peak_filter: NULL handle, negative size, leading dimension below M or window below -1");
        return SGPR_E_INVALID;
    }
    if (flags & ~SGPR_TOPK_CAUSAL) {
        set_error("sgpr_peak_filter: unknown flag bits " + std::to_string(flags & ~SGPR_TOPK_CAUSAL));
        return SGPR_E_INVALID;
    }
    if (!peak_radius_ok("sgpr_peak_filter", radius) || !row0_ok("sgpr_peak_filter", row0, R)) return SGPR_E_INVALID;
    if (R > 0 && M > 0 && (!d_score || !d_out)) {          // (an empty result needs no buffers)
        set_error("sgpr_peak_filter: NULL argument");
        return SGPR_E_INVALID;
    }
    if (R == 0 || M == 0) return SGPR_OK;
    const ScoreBlock block = {d_score, R, M, ld};
    DeviceGuard guard(h->device);
    return launch_peak_filter(block, eligible(d_row_self, row0, window, flags), radius, d_out, ldo,
                              static_cast<hipStream_t>(stream));
}

size_t sgpr_score_peak_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int k, int radius,
                                            int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > SGPR_TOPK_LARGE_MAX || L < 1 || L > SGPR_SEQ_MAX_LEN || ctx < 0 || ctx > R ||
        radius < 0 || radius > SGPR_PEAK_MAX_RADIUS || (flags & ~kSeqFlags) ||
        !(flags & (SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)))
        return 0;
    if (R == ctx || M == 0) return 0;
    return row_blocks_ws_bytes(h, R, M, rank_head_bytes(R, M, L, peak_stages(L, radius, flags)), L - 1);
}

int sgpr_score_peak_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L, int radius, int k,
                         float* d_values, int32_t* d_indices, unsigned char* d_dirs, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
    if (!h || R < 0 || M < 0) {
        set_error("sgpr_score_peak_topk: NULL handle or negative count");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok("sgpr_score_peak_topk", R, ctx, L, flags, kSeqFlags)) return SGPR_E_INVALID;
    if (!peak_radius_ok("sgpr_score_peak_topk", radius)) return SGPR_E_INVALID;
    if ((R > ctx && (!d_values || !d_indices)) || (R > ctx && M > 0 && (!d_pooled_rows || !d_pooled_cols))) {
        set_error("sgpr_score_peak_topk: NULL argument");
        return SGPR_E_INVALID;
    }
    if (!topk_large_args_ok("sgpr_score_peak_topk", R, k, flags & SGPR_TOPK_CAUSAL, row0)) return SGPR_E_INVALID;
    if (!workspace_ok("sgpr_score_peak_topk", sgpr_score_peak_topk_workspace_bytes(h, R, M, ctx, L, k, radius, flags),
                      d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == ctx) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const ListOut out = {d_values, d_indices, k, d_dirs};
    return rank_row_blocks(h, rect, seq_spec(ctx, L, flags), eligible(d_row_self, row0, window, flags), out,
                           peak_stages(L, radius, flags), d_workspace, workspace_bytes, stream);
}

// ---- sgpr_seq_path_filter / sgpr_score_path_topk: the path-set score filter (seq_path_kernel) on a resident matrix,
//      and on sgpr_score_peak_topk's row blocks in place of the diagonal filter (the peak step only when radius > 0)
static bool seq_paths_ok(const char* fn, const int32_t* h_offsets, int n_paths, int L) {
    if (n_paths < 1 || n_paths > SGPR_SEQ_MAX_PATHS) {
        set_error(std::string(fn) + ": n_paths must lie in 1.." + std::to_string(SGPR_SEQ_MAX_PATHS));
        return false;
    }
    if (!h_offsets) {
        set_error(std::string(fn) + ": NULL path table");
        return false;
    }
    for (int p = 0; p < n_paths; ++p) {
        const int32_t* off = h_offsets + (size_t)p * L;
        if (off[0] != 0) {
            set_error(std::string(fn) + ": path " + std::to_string(p) + " does not start at offset 0");
            return false;
        }
        for (int d = 1; d < L; ++d)
            if (off[d] < off[d - 1]) {
                set_error(std::string(fn) + ": path " + std::to_string(p) + " has a decreasing step at d = " +
                          std::to_string(d));
                return false;
            }
        if (off[L - 1] > SGPR_SEQ_PATH_MAX_OFFSET) {
            set_error(std::string(fn) + ": path " + std::to_string(p) + " has an offset above " +
                      std::to_string(SGPR_SEQ_PATH_MAX_OFFSET));
            return false;
        }
    }
    return true;
}

int sgpr_seq_path_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx, int L, int flags,
                         const int32_t* h_offsets, int n_paths, float* d_out, int64_t ldo, unsigned char* d_code,
                         void* stream) {
    if (!h || R < 0 || M < 0 || ld < M || ldo < M) {
        set_error("sgpr_seq_path_filter: NULL handle, negative size or leading dimension below M");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok("sgpr_seq_path_filter", R, ctx, L, flags, SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)) return SGPR_E_INVALID;
    if (!seq_paths_ok("sgpr_seq_path_filter", h_offsets, n_paths, L)) return SGPR_E_INVALID;
    if (R > ctx && M > 0 && (!d_score || !d_out)) {       // (an empty result needs no buffers)
        set_error("sgpr_seq_path_filter: NULL argument");
        return SGPR_E_INVALID;
    }
    if (R == ctx || M == 0) return SGPR_OK;
    const ScoreBlock block = {d_score, R, M, ld};
    const FilterOut out = {d_out, ldo, d_code, ldo};
    DeviceGuard guard(h->device);
    return launch_seq_path_filter(block, seq_spec(ctx, L, flags).paths(h_offsets, n_paths), out,
                                  static_cast<hipStream_t>(stream));
}

size_t sgpr_score_path_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int n_paths, int k,
                                            int radius, int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > SGPR_TOPK_LARGE_MAX || L < 1 || L > SGPR_SEQ_MAX_LEN || ctx < 0 || ctx > R ||
        n_paths < 1 || n_paths > SGPR_SEQ_MAX_PATHS || radius < 0 || radius > SGPR_PEAK_MAX_RADIUS ||
        (flags & ~kSeqFlags) || !(flags & (SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)))
        return 0;
    if (R == ctx || M == 0) return 0;
    return row_blocks_ws_bytes(h, R, M, rank_head_bytes(R, M, L, path_stages(L, n_paths, radius, flags)), L - 1);
}

int sgpr_score_path_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L,
                         const int32_t* h_offsets, int n_paths, int radius, int k, float* d_values, int32_t* d_indices,
                         unsigned char* d_codes, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!h || R < 0 || M < 0) {
        set_error("sgpr_score_path_topk: NULL handle or negative count");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok("sgpr_score_path_topk", R, ctx, L, flags, kSeqFlags)) return SGPR_E_INVALID;
    if (!seq_paths_ok("sgpr_score_path_topk", h_offsets, n_paths, L)) return SGPR_E_INVALID;
    if (!peak_radius_ok("sgpr_score_path_topk", radius)) return SGPR_E_INVALID;
    if ((R > ctx && (!d_values || !d_indices)) || (R > ctx && M > 0 && (!d_pooled_rows || !d_pooled_cols))) {
        set_error("sgpr_score_path_topk: NULL argument");
        return SGPR_E_INVALID;
    }
    if (!topk_large_args_ok("sgpr_score_path_topk", R, k, flags & SGPR_TOPK_CAUSAL, row0)) return SGPR_E_INVALID;
    if (!workspace_ok("sgpr_score_path_topk",
                      sgpr_score_path_topk_workspace_bytes(h, R, M, ctx, L, n_paths, k, radius, flags), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == ctx) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const ListOut out = {d_values, d_indices, k, d_codes};
    return rank_row_blocks(h, rect, seq_spec(ctx, L, flags).paths(h_offsets, n_paths),
                           eligible(d_row_self, row0, window, flags), out, path_stages(L, n_paths, radius, flags),
                           d_workspace, workspace_bytes, stream);
}

// ---- sgpr_session_filter / sgpr_score_session_topk: the session-aware path-set filter (session_kernel) on a resident
//      matrix, and on sgpr_score_path_topk's row blocks (radius 0) with the row table shifted per block; the window is the
//      filter's, so the selection runs without one
static bool session_paths_ok(const char* fn, const int32_t* h_offsets, int n_paths, int L) {
    if (n_paths == 0 && !h_offsets) return true;          // the unit diagonal
    if (n_paths == 0) {
        set_error(std::string(fn) + ": a path table with n_paths = 0");
        return false;
    }
    return seq_paths_ok(fn, h_offsets, n_paths, L);
}

int sgpr_session_filter(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx, int L, int flags,
                        const int32_t* h_offsets, int n_paths, const int32_t* h_row_starts, int n_row_sessions,
                        const int32_t* h_col_starts, int n_col_sessions, const int32_t* d_row_self, int row0, int window,
                        float* d_out, int64_t ldo, unsigned char* d_code, void* stream) {
    const char* fn = "sgpr_session_filter";
    if (!h || R < 0 || M < 0 || ld < M || ldo < M || window < -1) {
        set_error("sgpr_session_filter: NULL handle, negative size, leading dimension below M or window below -1");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok(fn, R, ctx, L, flags, SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)) return SGPR_E_INVALID;
    if (!session_paths_ok(fn, h_offsets, n_paths, L)) return SGPR_E_INVALID;
    if (!session_table_ok(fn, "row", h_row_starts, n_row_sessions, R) ||
        !session_table_ok(fn, "column", h_col_starts, n_col_sessions, M) || !row0_ok(fn, row0, R))
        return SGPR_E_INVALID;
    if (R > ctx && M > 0 && (!d_score || !d_out)) {       // (an empty result needs no buffers)
        set_error("sgpr_session_filter: NULL argument");
        return SGPR_E_INVALID;
    }
    if (R == ctx || M == 0) return SGPR_OK;
    const ScoreBlock block = {d_score, R, M, ld};
    const SeqSpec seq = seq_spec(ctx, L, flags).paths(h_offsets, n_paths)
                            .sessions(h_row_starts, n_row_sessions, h_col_starts, n_col_sessions);
    const FilterOut out = {d_out, ldo, d_code, ldo};
    DeviceGuard guard(h->device);
    return launch_session_filter(block, seq, eligible(d_row_self, row0, window, 0), out, static_cast<hipStream_t>(stream));
}

size_t sgpr_score_session_topk_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int n_paths, int k,
                                               int flags, int n_row_sessions, int n_col_sessions) {
    if (n_paths < 0 || n_row_sessions < 0 || n_row_sessions > SGPR_SESSION_MAX || n_col_sessions < 0 ||
        n_col_sessions > SGPR_SESSION_MAX)
        return 0;
    return sgpr_score_path_topk_workspace_bytes(h, R, M, ctx, L, std::max(n_paths, 1), k, 0, flags);
}

int sgpr_score_session_topk(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                            int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L,
                            const int32_t* h_offsets, int n_paths, const int32_t* h_row_starts, int n_row_sessions,
                            const int32_t* h_col_starts, int n_col_sessions, int k, float* d_values, int32_t* d_indices,
                            unsigned char* d_codes, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "sgpr_score_session_topk";
    if (!h || R < 0 || M < 0 || window < -1) {
        set_error("sgpr_score_session_topk: NULL handle, negative count or window below -1");
        return SGPR_E_INVALID;
    }
    if (!seq_args_ok(fn, R, ctx, L, flags, kSeqFlags)) return SGPR_E_INVALID;
    if (!session_paths_ok(fn, h_offsets, n_paths, L)) return SGPR_E_INVALID;
    if (!session_table_ok(fn, "row", h_row_starts, n_row_sessions, R) ||
        !session_table_ok(fn, "column", h_col_starts, n_col_sessions, M))
        return SGPR_E_INVALID;
    if ((R > ctx && (!d_values || !d_indices)) || (R > ctx && M > 0 && (!d_pooled_rows || !d_pooled_cols))) {
        set_error("sgpr_score_session_topk: NULL argument");
        return SGPR_E_INVALID;
    }
    if (!topk_large_args_ok(fn, R, k, flags & SGPR_TOPK_CAUSAL, row0)) return SGPR_E_INVALID;
    if (!workspace_ok(fn, sgpr_score_session_topk_workspace_bytes(h, R, M, ctx, L, n_paths, k, flags, n_row_sessions,
                                                                  n_col_sessions),
                      d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == ctx) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const SeqSpec seq = seq_spec(ctx, L, flags).paths(h_offsets, n_paths)
                            .sessions(h_row_starts, n_row_sessions, h_col_starts, n_col_sessions);
    const ListOut out = {d_values, d_indices, k, d_codes};
    return rank_row_blocks(h, rect, seq, eligible(d_row_self, row0, window, flags), out, session_stages(L, n_paths, flags),
                           d_workspace, workspace_bytes, stream);
}

// ---- sgpr_score_mine / sgpr_mine_rows: sgpr_score_topk's split (fused on the production handle, 64 MB score blocks
//      and sgpr_mine_rows' kernel on the others) with the pose-class condition of the mined pairs
static const int kMineFlags = SGPR_TOPK_CAUSAL | SGPR_MINE_NEGATIVES | SGPR_MINE_POSITIVES;

static bool mine_flags_ok(int flags) {
    const int mode = flags & (SGPR_MINE_NEGATIVES | SGPR_MINE_POSITIVES);
    return !(flags & ~kMineFlags) && (mode == SGPR_MINE_NEGATIVES || mode == SGPR_MINE_POSITIVES);
}

static bool mine_args_ok(const char* fn, const sgpr_handle* h, int R, int M, int row0, int flags, const MineSpec& mine,
                         const ListOut& out) {
    const double d_pos = mine.d_pos, d_neg = mine.d_neg;
    if (!h || R < 0 || M < 0 || !mine.col_pose || !out.val || !out.idx) {
        set_error(std::string(fn) + ": NULL argument or negative count");
        return false;
    }
    if (out.k < 1 || out.k > 16) {
        set_error(std::string(fn) + ": k must lie in 1..16");
        return false;
    }
    if (!mine_flags_ok(flags)) {
        set_error(std::string(fn) + ": flags must hold exactly one of SGPR_MINE_NEGATIVES / SGPR_MINE_POSITIVES and no "
                  "unknown bit (got " + std::to_string(flags) + ")");
        return false;
    }
    if (d_pos != d_pos || d_neg != d_neg || d_pos < 0.0 || d_pos > d_neg) {
        // (a negative d_pos: the squared rule would take s2 < d_pos^2 as positive, PairSet._targets' d <= d_pos never)
        set_error(std::string(fn) + ": d_pos / d_neg NaN, d_pos < 0 or d_pos > d_neg");
        return false;
    }
    return row0_ok(fn, row0, R);
}

size_t sgpr_score_mine_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags) {
    if (!h || R < 0 || M < 0 || k < 1 || k > 16 || !mine_flags_ok(flags)) return 0;
    if (R == 0 || M == 0) return 0;
    if (has_fused_epilogues(h)) return score_mine_ws_bytes(h, R, M, k);
    return row_blocks_ws_bytes(h, R, M, 0);
}

int sgpr_score_mine(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                    const double* d_col_pose_xz, const double* d_row_pose_xz, const int32_t* d_row_self, int row0,
                    int window, int flags, double d_pos, double d_neg, int k, float* d_values, int32_t* d_indices,
                    void* d_workspace, size_t workspace_bytes, void* stream) {
    const MineSpec mine = mine_spec(flags, d_col_pose_xz, d_row_pose_xz, d_pos, d_neg);
    const ListOut out = {d_values, d_indices, k, nullptr};
    if (!mine_args_ok("sgpr_score_mine", h, R, M, row0, flags, mine, out)) return SGPR_E_INVALID;
    if (!d_pooled_rows || !d_pooled_cols) {
        set_error("sgpr_score_mine: NULL pooled array");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_mine", sgpr_score_mine_workspace_bytes(h, R, M, k, flags), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    if (R == 0) return SGPR_OK;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const Eligible elig = eligible(d_row_self, row0, window, flags);
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (M == 0 || has_fused_epilogues(h)) return launch_score_mine(h, rect, elig, mine, out, d_workspace, s);
    auto select = [&](const ScoreBlock& block, unsigned char*, int r0) {
        return launch_mine_rows(block, elig.from(r0), mine.from(r0), out.at(r0), h->d_status, s);
    };
    return score_row_blocks(h, rect, 0, d_workspace, workspace_bytes, stream, select);
}

size_t sgpr_mine_rows_workspace_bytes(const sgpr_handle* h, int R, int M, int k, int flags) {
    (void)h;
    (void)R;
    (void)M;
    (void)k;
    (void)flags;
    return 0;
}

int sgpr_mine_rows(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const double* d_col_pose_xz,
                   const double* d_row_pose_xz, const int32_t* d_row_self, int row0, int window, int flags, double d_pos,
                   double d_neg, int k, float* d_values, int32_t* d_indices, void* d_workspace, size_t workspace_bytes,
                   void* stream) {
    (void)d_workspace;
    (void)workspace_bytes;
    const MineSpec mine = mine_spec(flags, d_col_pose_xz, d_row_pose_xz, d_pos, d_neg);
    const ListOut out = {d_values, d_indices, k, nullptr};
    if (!mine_args_ok("sgpr_mine_rows", h, R, M, row0, flags, mine, out)) return SGPR_E_INVALID;
    if (!d_score || ld < M) {
        set_error("sgpr_mine_rows: NULL score matrix or leading dimension below M");
        return SGPR_E_INVALID;
    }
    if (R == 0) return SGPR_OK;
    const ScoreBlock block = {d_score, R, M, ld};
    DeviceGuard guard(h->device);
    return launch_mine_rows(block, eligible(d_row_self, row0, window, flags), mine, out, h->d_status,
                            static_cast<hipStream_t>(stream));
}

// ---- sgpr_score_above / sgpr_rows_above: the fused two-pass kernel on the production handle; the other handles score
//      bounded row blocks with their own tail and select from each block, positions continuing on the device
static bool above_args_ok(const char* fn, const sgpr_handle* h, int R, int M, int row0, int flags, float threshold,
                          const RangeOut& out) {
    if (!h || R < 0 || M < 0 || out.cap < 0 || !out.count || (out.cap > 0 && (!out.rows || !out.cols || !out.vals))) {
        set_error(std::string(fn) + ": NULL argument, negative count or negative capacity");
        return false;
    }
    if (flags & ~SGPR_TOPK_CAUSAL) {
        set_error(std::string(fn) + ": unknown flag bits " + std::to_string(flags & ~SGPR_TOPK_CAUSAL));
        return false;
    }
    if (threshold != threshold) {
        set_error(std::string(fn) + ": the threshold is NaN");
        return false;
    }
    return row0_ok(fn, row0, R);
}

// head of sgpr_score_above's row-block path: cnt [rb] i32 | row_ptr [R + 1] i64 (used when the caller passes none)
static size_t above_head_bytes(int R, int M) {
    return a256((size_t)score_block_rows(R, M) * 4) + a256((size_t)(R + 1) * 8);
}

size_t sgpr_score_above_workspace_bytes(const sgpr_handle* h, int R, int M, int flags) {
    if (!h || R < 0 || M < 0 || (flags & ~SGPR_TOPK_CAUSAL)) return 0;
    if (R == 0 || M == 0) return 0;
    if (has_fused_epilogues(h)) return score_above_ws_bytes(h, R, M);
    return row_blocks_ws_bytes(h, R, M, above_head_bytes(R, M));
}

int sgpr_score_above(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                     const int32_t* d_row_self, int row0, int window, int flags, float threshold, int32_t* d_rows,
                     int32_t* d_cols, float* d_values, int64_t capacity, int64_t* d_row_ptr, unsigned long long* d_count,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
    // (the output bundle carries the handle's status word: read only once the checks have seen h)
    RangeOut out = range_out(d_rows, d_cols, d_values, nullptr, capacity, d_row_ptr, d_count, h ? h->d_status : nullptr);
    if (!above_args_ok("sgpr_score_above", h, R, M, row0, flags, threshold, out)) return SGPR_E_INVALID;
    if (R > 0 && M > 0 && (!d_pooled_rows || !d_pooled_cols)) {
        set_error("sgpr_score_above: NULL pooled vectors");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_above", sgpr_score_above_workspace_bytes(h, R, M, flags), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const Eligible elig = eligible(d_row_self, row0, window, flags);
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == 0 || M == 0 || has_fused_epilogues(h))
        return launch_score_above(h, rect, elig, threshold, out.at(0, d_workspace), s);
    const size_t cnt_bytes = a256((size_t)score_block_rows(R, M) * 4);
    if (!out.row_ptr) out.row_ptr = reinterpret_cast<int64_t*>(row_blocks_head(d_workspace, R, M) + cnt_bytes);
    auto select = [&](const ScoreBlock& block, unsigned char* cnt, int r0) {
        return launch_rows_above(block, elig.from(r0), threshold, out.at(r0, cnt), s);
    };
    return score_row_blocks(h, rect, above_head_bytes(R, M), d_workspace, workspace_bytes, stream, select);
}

size_t sgpr_rows_above_workspace_bytes(const sgpr_handle* h, int R, int M) {
    if (!h || R < 0 || M < 0 || R == 0 || M == 0) return 0;
    return rows_above_ws_bytes(R);
}

int sgpr_rows_above(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, const int32_t* d_row_self,
                    int row0, int window, int flags, float threshold, int32_t* d_rows, int32_t* d_cols, float* d_values,
                    int64_t capacity, int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace,
                    size_t workspace_bytes, void* stream) {
    RangeOut out = range_out(d_rows, d_cols, d_values, nullptr, capacity, d_row_ptr, d_count, h ? h->d_status : nullptr);
    if (!above_args_ok("sgpr_rows_above", h, R, M, row0, flags, threshold, out)) return SGPR_E_INVALID;
    if (ld < M || (R > 0 && M > 0 && !d_score)) {
        set_error("sgpr_rows_above: NULL score or ld < M");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_rows_above", sgpr_rows_above_workspace_bytes(h, R, M), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == 0 || M == 0) return launch_above_empty(R, d_row_ptr, d_count, s);
    unsigned char* cnt = static_cast<unsigned char*>(d_workspace);
    if (!out.row_ptr) out.row_ptr = reinterpret_cast<int64_t*>(cnt + a256((size_t)R * 4));
    const ScoreBlock block = {d_score, R, M, ld};
    return launch_rows_above(block, eligible(d_row_self, row0, window, flags), threshold, out.at(0, cnt), s);
}

// ---- sgpr_seq_rows_above / sgpr_score_seq_above: the range selection on the sequence-matched score (seq_above_kernel,
//      sgpr_seq.hip) on a resident matrix, and on sgpr_score_seq_topk's row blocks with context - no Q or dir block
static bool seq_above_args_ok(const char* fn, const sgpr_handle* h, int R, int M, int ctx, int row0, int flags, int L,
                              float threshold, const RangeOut& out) {
    if (!above_args_ok(fn, h, R, M, row0, flags & SGPR_TOPK_CAUSAL, threshold, out)) return false;
    return seq_args_ok(fn, R, ctx, L, flags, kSeqFlags);
}

static bool seq_query_ok(const sgpr_handle* h, int R, int M, int ctx, int L, int flags) {
    return h && R >= 0 && M >= 0 && L >= 1 && L <= SGPR_SEQ_MAX_LEN && ctx >= 0 && ctx <= R && !(flags & ~kSeqFlags) &&
           (flags & (SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE));
}

// workspace of sgpr_seq_rows_above: seg, cnt (seq_above_ws_bytes) | row_ptr [R - ctx + 1] i64 (the caller passes none)
size_t sgpr_seq_rows_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx) {
    if (!h || R < 0 || M < 0 || ctx < 0 || ctx > R || R == ctx || M == 0) return 0;
    return seq_above_ws_bytes(R - ctx, M) + a256((size_t)(R - ctx + 1) * 8);
}

int sgpr_seq_rows_above(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx,
                        const int32_t* d_row_self, int row0, int window, int flags, int L, float threshold,
                        int32_t* d_rows, int32_t* d_cols, float* d_values, unsigned char* d_dirs, int64_t capacity,
                        int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
    RangeOut out = range_out(d_rows, d_cols, d_values, d_dirs, capacity, d_row_ptr, d_count, h ? h->d_status : nullptr);
    if (!seq_above_args_ok("sgpr_seq_rows_above", h, R, M, ctx, row0, flags, L, threshold, out)) return SGPR_E_INVALID;
    if (ld < M || (R > ctx && M > 0 && !d_score)) {
        set_error("sgpr_seq_rows_above: NULL score or ld < M");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_seq_rows_above", sgpr_seq_rows_above_workspace_bytes(h, R, M, ctx), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == ctx || M == 0) return launch_above_empty(R - ctx, d_row_ptr, d_count, s);
    unsigned char* ws = static_cast<unsigned char*>(d_workspace);
    if (!out.row_ptr) out.row_ptr = reinterpret_cast<int64_t*>(ws + seq_above_ws_bytes(R - ctx, M));
    const ScoreBlock block = {d_score, R, M, ld};
    return launch_seq_above(block, seq_spec(ctx, L, flags), eligible(d_row_self, row0, window, flags), threshold,
                            out.at(0, ws), s);
}

// head of sgpr_score_seq_above: the call's f16 range (a float4) | seg, cnt for one block | row_ptr [R - ctx + 1] i64
// (used when the caller passes none)
static size_t seq_above_head_bytes(int R, int M, int ctx, int L) {
    return 256 + seq_above_ws_bytes(score_block_rows(R, M, L - 1), M) + a256((size_t)(R - ctx + 1) * 8);
}

// the range pipeline of sgpr_score_seq_above (seq_above_kernel) and, `sessions`, sgpr_score_session_above
// (session_above_kernel) on the ranking pipeline's row blocks with context - no Q or code block.  Arguments and
// workspace already checked; out.row_ptr == nullptr: the head holds it
static int range_row_blocks(const sgpr_handle* h, const PooledRect& p, const SeqSpec& seq, bool sessions,
                            const Eligible& elig, float threshold, const RangeOut& out, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
    const int R = p.R, M = p.M, ctx = seq.ctx, L = seq.L;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == ctx || M == 0) return launch_above_empty(R - ctx, out.row_ptr, out.count, s);
    unsigned char* crng = row_blocks_head(d_workspace, R, M, L - 1);
    RangeOut call = out;
    if (!call.row_ptr)
        call.row_ptr = reinterpret_cast<int64_t*>(crng + 256 + seq_above_ws_bytes(score_block_rows(R, M, L - 1), M));
    auto select = [&](const ScoreBlock& scored, unsigned char* head, int r0) {
        const BlockView v(scored, r0, ctx, L);
        if (v.no <= 0) return (int)SGPR_OK;               // context rows only
        // row_self / row0 and the row table move with the rectangle
        const ShiftedSeq sq(seq, v);
        const RangeOut o = call.at(v.first - ctx, head + 256);
        return sessions ? launch_session_above(v.rect, sq, elig.from(v.base), threshold, o, s)
                        : launch_seq_above(v.rect, sq, elig.from(v.base), threshold, o, s);
    };
    return score_row_blocks(h, p, seq_above_head_bytes(R, M, ctx, L), d_workspace, workspace_bytes, stream, select,
                            reinterpret_cast<float*>(crng), L - 1);
}

size_t sgpr_score_seq_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int flags) {
    if (!seq_query_ok(h, R, M, ctx, L, flags)) return 0;
    if (R == ctx || M == 0) return 0;
    return row_blocks_ws_bytes(h, R, M, seq_above_head_bytes(R, M, ctx, L), L - 1);
}

int sgpr_score_seq_above(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L, float threshold,
                         int32_t* d_rows, int32_t* d_cols, float* d_values, unsigned char* d_dirs, int64_t capacity,
                         int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
    const RangeOut out = range_out(d_rows, d_cols, d_values, d_dirs, capacity, d_row_ptr, d_count,
                                   h ? h->d_status : nullptr);
    if (!seq_above_args_ok("sgpr_score_seq_above", h, R, M, ctx, row0, flags, L, threshold, out)) return SGPR_E_INVALID;
    if (R > ctx && M > 0 && (!d_pooled_rows || !d_pooled_cols)) {
        set_error("sgpr_score_seq_above: NULL pooled vectors");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_seq_above", sgpr_score_seq_above_workspace_bytes(h, R, M, ctx, L, flags), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    return range_row_blocks(h, rect, seq_spec(ctx, L, flags), false, eligible(d_row_self, row0, window, flags), threshold,
                            out, d_workspace, workspace_bytes, stream);
}

// ---- sgpr_session_rows_above / sgpr_score_session_above: the range selection on the session-aware path-set score with a
//      minimum term count (session_above_kernel) on a resident matrix, and on
//      sgpr_score_seq_above's row blocks with the row table shifted per block as sgpr_score_session_topk shifts it
static bool session_above_args_ok(const char* fn, const sgpr_handle* h, int R, int M, int row0, int window, int flags,
                                  const SeqSpec& seq, float threshold, const RangeOut& out) {
    if (!seq_above_args_ok(fn, h, R, M, seq.ctx, row0, flags, seq.L, threshold, out)) return false;
    if (window < -1) {
        set_error(std::string(fn) + ": window below -1");
        return false;
    }
    if (!session_paths_ok(fn, seq.offsets, seq.n_paths, seq.L)) return false;
    if (!session_table_ok(fn, "row", seq.row_starts, seq.n_row, R) ||
        !session_table_ok(fn, "column", seq.col_starts, seq.n_col, M))
        return false;
    if (seq.min_terms < 1 || seq.min_terms > seq.L) {
        set_error(std::string(fn) + ": min_terms must lie in 1..L, got " + std::to_string(seq.min_terms));
        return false;
    }
    return true;
}

size_t sgpr_session_rows_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx) {
    return sgpr_seq_rows_above_workspace_bytes(h, R, M, ctx);
}

int sgpr_session_rows_above(const sgpr_handle* h, const float* d_score, int R, int M, int64_t ld, int ctx,
                            const int32_t* d_row_self, int row0, int window, int flags, int L, const int32_t* h_offsets,
                            int n_paths, const int32_t* h_row_starts, int n_row_sessions, const int32_t* h_col_starts,
                            int n_col_sessions, int min_terms, float threshold, int32_t* d_rows, int32_t* d_cols,
                            float* d_values, unsigned char* d_codes, int64_t capacity, int64_t* d_row_ptr,
                            unsigned long long* d_count, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "sgpr_session_rows_above";
    const SeqSpec seq = seq_spec(ctx, L, flags, min_terms).paths(h_offsets, n_paths)
                            .sessions(h_row_starts, n_row_sessions, h_col_starts, n_col_sessions);
    RangeOut out = range_out(d_rows, d_cols, d_values, d_codes, capacity, d_row_ptr, d_count, h ? h->d_status : nullptr);
    if (!session_above_args_ok(fn, h, R, M, row0, window, flags, seq, threshold, out)) return SGPR_E_INVALID;
    if (ld < M || (R > ctx && M > 0 && !d_score)) {
        set_error("sgpr_session_rows_above: NULL score or ld < M");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok(fn, sgpr_session_rows_above_workspace_bytes(h, R, M, ctx), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == ctx || M == 0) return launch_above_empty(R - ctx, d_row_ptr, d_count, s);
    unsigned char* ws = static_cast<unsigned char*>(d_workspace);
    if (!out.row_ptr) out.row_ptr = reinterpret_cast<int64_t*>(ws + seq_above_ws_bytes(R - ctx, M));
    const ScoreBlock block = {d_score, R, M, ld};
    return launch_session_above(block, seq, eligible(d_row_self, row0, window, flags), threshold, out.at(0, ws), s);
}

size_t sgpr_score_session_above_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int n_paths, int flags,
                                                int n_row_sessions, int n_col_sessions) {
    if (n_paths < 0 || n_paths > SGPR_SEQ_MAX_PATHS || n_row_sessions < 0 || n_row_sessions > SGPR_SESSION_MAX ||
        n_col_sessions < 0 || n_col_sessions > SGPR_SESSION_MAX)
        return 0;
    return sgpr_score_seq_above_workspace_bytes(h, R, M, ctx, L, flags);   // (the halo lives in LDS, not here)
}

int sgpr_score_session_above(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                             int ctx, const int32_t* d_row_self, int row0, int window, int flags, int L,
                             const int32_t* h_offsets, int n_paths, const int32_t* h_row_starts, int n_row_sessions,
                             const int32_t* h_col_starts, int n_col_sessions, int min_terms, float threshold,
                             int32_t* d_rows, int32_t* d_cols, float* d_values, unsigned char* d_codes, int64_t capacity,
                             int64_t* d_row_ptr, unsigned long long* d_count, void* d_workspace, size_t workspace_bytes,
                             void* stream) {
    const char* fn = "sgpr_score_session_above";
    const SeqSpec seq = seq_spec(ctx, L, flags, min_terms).paths(h_offsets, n_paths)
                            .sessions(h_row_starts, n_row_sessions, h_col_starts, n_col_sessions);
    const RangeOut out = range_out(d_rows, d_cols, d_values, d_codes, capacity, d_row_ptr, d_count,
                                   h ? h->d_status : nullptr);
    if (!session_above_args_ok(fn, h, R, M, row0, window, flags, seq, threshold, out)) return SGPR_E_INVALID;
    if (R > ctx && M > 0 && (!d_pooled_rows || !d_pooled_cols)) {
        set_error("sgpr_score_session_above: NULL pooled vectors");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok(fn, sgpr_score_session_above_workspace_bytes(h, R, M, ctx, L, n_paths, flags, n_row_sessions,
                                                                   n_col_sessions),
                      d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    return range_row_blocks(h, rect, seq, true, eligible(d_row_self, row0, window, flags), threshold, out, d_workspace,
                            workspace_bytes, stream);
}

// ---- sgpr_score_positives / sgpr_score_threshold_counts: the fused evaluation epilogues on the production handle; the
//      other handles score bounded row blocks with their own tail and run the matrix kernels on each block, row0
//      advancing, the blocks' results added up on the device
static bool eval_args_ok(const char* fn, const sgpr_handle* h, const float* rows, int R, const float* cols, int M,
                         int row0, const double* pose, const signed char* gt, int64_t ldg) {
    if (!h || R < 0 || M < 0 || (R > 0 && M > 0 && (!rows || !cols)) || (!pose && !gt) || (gt && !pose && ldg < M)) {
        set_error(std::string(fn) + ": NULL argument, negative count, no ground truth or ldg below M");
        return false;
    }
    return row0_ok(fn, row0, R);
}

static PairTruth eval_truth(int row0, const double* pose, double d_pos, double d_neg, const signed char* gt, int64_t ldg) {
    PairTruth t;
    memset(&t, 0, sizeof(t));
    t.row0 = row0;
    t.pose = pose;
    t.d_pos = d_pos;
    t.d_neg = d_neg;
    t.gt = pose ? nullptr : gt;
    t.ldg = ldg;
    return t;
}

// the truth of the rows from `r` on, whose explicit labels start `g` label rows in
static PairTruth truth_from(const PairTruth& t, int r, int g) {
    PairTruth tb = t;
    tb.row0 += r;
    if (tb.gt) tb.gt += (int64_t)g * t.ldg;
    return tb;
}

// head of sgpr_score_threshold_counts' row-block path: the counting slabs (every block's counts fold into d_out)
static size_t counts_head_bytes(const sgpr_handle* h, int T) {
    return a256(sgpr_pair_threshold_counts_workspace_bytes(h, T));
}

size_t sgpr_score_positives_workspace_bytes(const sgpr_handle* h, int R, int M) {
    if (!h || R < 0 || M < 0 || R == 0 || M == 0) return 0;
    if (has_fused_epilogues(h)) return score_eval_ws_bytes(h, R, M, -1);
    return row_blocks_ws_bytes(h, R, M, 0);
}

size_t sgpr_score_threshold_counts_workspace_bytes(const sgpr_handle* h, int R, int M, int T) {
    if (!h || R < 0 || M < 0 || T < 0 || T > SGPR_SCORE_COUNT_MAX_THRESHOLDS || R == 0 || M == 0) return 0;
    if (has_fused_epilogues(h)) return score_eval_ws_bytes(h, R, M, T);
    return row_blocks_ws_bytes(h, R, M, counts_head_bytes(h, T));
}

int sgpr_score_positives(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                         int row0, const double* d_pose_xz, double d_pos, double d_neg, const signed char* d_gt,
                         int64_t ldg, float* d_out, int64_t capacity, unsigned long long* d_count,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!eval_args_ok("sgpr_score_positives", h, d_pooled_rows, R, d_pooled_cols, M, row0, d_pose_xz, d_gt, ldg))
        return SGPR_E_INVALID;
    if (!d_count || capacity < 0 || (capacity > 0 && !d_out)) {
        set_error("sgpr_score_positives: NULL count buffer or capacity without an output buffer");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_positives", sgpr_score_positives_workspace_bytes(h, R, M), d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PairTruth truth = eval_truth(row0, d_pose_xz, d_pos, d_neg, d_gt, ldg);
    float* out = capacity > 0 ? d_out : nullptr;
    if ((int64_t)R * M == 0 || has_fused_epilogues(h))
        return launch_score_eval(h, d_pooled_rows, R, d_pooled_cols, M, truth, out, capacity, d_count, nullptr, -1, nullptr,
                                 0, nullptr, nullptr, d_workspace, s);
    hipError_t e = hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_score_positives: memset");
    auto count = [&](const ScoreBlock& block, unsigned char*, int r0) {
        return launch_pair_positives_more(h, block.score, block.R, M, M, truth_from(truth, r0, r0), out, capacity, d_count,
                                          s);
    };
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    return score_row_blocks(h, rect, 0, d_workspace, workspace_bytes, stream, count);
}

int sgpr_score_threshold_counts(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols,
                                int M, int row0, const double* d_pose_xz, double d_pos, double d_neg,
                                const signed char* d_gt, int64_t ldg, const float* d_thresholds, int T,
                                const sgpr_rank_group* d_rank, int groups_per_threshold,
                                const unsigned long long* d_at_least, unsigned long long* d_out,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!eval_args_ok("sgpr_score_threshold_counts", h, d_pooled_rows, R, d_pooled_cols, M, row0, d_pose_xz, d_gt, ldg))
        return SGPR_E_INVALID;
    if (!d_out || T < 0 || T > SGPR_SCORE_COUNT_MAX_THRESHOLDS || (T > 0 && !d_thresholds)) {
        set_error("sgpr_score_threshold_counts: 0.." + std::to_string(SGPR_SCORE_COUNT_MAX_THRESHOLDS) +
                  " thresholds and an output buffer");
        return SGPR_E_INVALID;
    }
    if (d_rank && (T < 1 || groups_per_threshold < 1 || !d_at_least)) {
        set_error("sgpr_score_threshold_counts: the ranking needs thresholds, >= 1 value group per threshold and the pair counts");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_threshold_counts", sgpr_score_threshold_counts_workspace_bytes(h, R, M, T), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PairTruth truth = eval_truth(row0, d_pose_xz, d_pos, d_neg, d_gt, ldg);
    if ((int64_t)R * M == 0 || has_fused_epilogues(h))
        return launch_score_eval(h, d_pooled_rows, R, d_pooled_cols, M, truth, nullptr, 0, nullptr, d_thresholds, T, d_rank,
                                 groups_per_threshold, d_at_least, d_out, d_workspace, s);
    hipError_t e = hipMemsetAsync(d_out, 0, (size_t)(T + 3) * sizeof(unsigned long long), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_score_threshold_counts: memset");
    auto count = [&](const ScoreBlock& block, unsigned char* head, int r0) {
        return launch_pair_counts_more(h, block.score, block.R, M, M, truth_from(truth, r0, r0), d_thresholds, T, d_rank,
                                       groups_per_threshold, d_at_least, d_out, reinterpret_cast<unsigned*>(head), 1, s);
    };
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    return score_row_blocks(h, rect, counts_head_bytes(h, T), d_workspace, workspace_bytes, stream, count);
}

// ---- sgpr_score_seq_positives / sgpr_score_seq_threshold_counts: the evaluation of the sequence-matched score on
//      sgpr_score_seq_topk's row blocks with context (every handle): each block is filtered into a Q block and handed
//      to the matrix kernels, row0 and d_gt advanced to the block's first output row - the wide-range path above with
//      the filter in between.  (The counting kernels carry a threshold tree and rank sums: they are not fused into the
//      filter.)
static bool seq_eval_args_ok(const char* fn, const sgpr_handle* h, const PooledRect& p, int ctx, int L, int flags,
                             const PairTruth& truth) {
    if (!h || p.R < 0 || p.M < 0 || (!truth.pose && !truth.gt) || (truth.gt && truth.ldg < p.M)) {
        set_error(std::string(fn) + ": NULL argument, negative count, no ground truth or ldg below M");
        return false;
    }
    if (!seq_args_ok(fn, p.R, ctx, L, flags, SGPR_SEQ_FORWARD | SGPR_SEQ_REVERSE)) return false;
    if (p.R > ctx && p.M > 0 && (!p.rows || !p.cols)) {
        set_error(std::string(fn) + ": NULL pooled vectors");
        return false;
    }
    return row0_ok(fn, truth.row0, p.R);
}

static bool seq_eval_query_ok(const sgpr_handle* h, int R, int M, int ctx, int L, int flags) {
    return seq_query_ok(h, R, M, ctx, L, flags) && !(flags & SGPR_TOPK_CAUSAL);
}

// head of the two calls: the call's f16 range (a float4) | Q block [rb][M] | (counts) the counting slabs
static size_t seq_eval_head_bytes(int R, int M, int L) {
    return 256 + a256((size_t)score_block_rows(R, M, L - 1) * M * sizeof(float));
}

size_t sgpr_score_seq_positives_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int flags) {
    if (!seq_eval_query_ok(h, R, M, ctx, L, flags) || R == ctx || M == 0) return 0;
    return row_blocks_ws_bytes(h, R, M, seq_eval_head_bytes(R, M, L), L - 1);
}

size_t sgpr_score_seq_threshold_counts_workspace_bytes(const sgpr_handle* h, int R, int M, int ctx, int L, int flags,
                                                       int T) {
    if (!seq_eval_query_ok(h, R, M, ctx, L, flags) || T < 0 || T > SGPR_SCORE_COUNT_MAX_THRESHOLDS || R == ctx || M == 0)
        return 0;
    return row_blocks_ws_bytes(h, R, M, seq_eval_head_bytes(R, M, L) + counts_head_bytes(h, T), L - 1);
}

extern "C++" {
// score_row_blocks with L - 1 context rows; each block with output rows is filtered into the Q block and
// consume(q, tail, first) sees Q of the call's rows [first, first + q.R) (ld M); tail: the head behind the Q block
template <class Consume>
static int seq_eval_blocks(const sgpr_handle* h, const PooledRect& p, const SeqSpec& seq, size_t head_bytes, void* ws,
                           size_t ws_bytes, void* stream, Consume&& consume) {
    const int M = p.M;
    const size_t q_bytes = a256((size_t)score_block_rows(p.R, M, seq.L - 1) * M * sizeof(float));
    float* crng = reinterpret_cast<float*>(row_blocks_head(ws, p.R, M, seq.L - 1));
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto filter = [&](const ScoreBlock& scored, unsigned char* head, int r0) {
        const BlockView v(scored, r0, seq.ctx, seq.L);
        if (v.no <= 0) return (int)SGPR_OK;               // context rows only
        const FilterOut q = {reinterpret_cast<float*>(head + 256), M, nullptr, M};
        const int rc = launch_seq_filter(v.rect, ShiftedSeq(seq, v), q, s);
        return rc != SGPR_OK ? rc : consume(ScoreBlock{q.out, v.no, M, M}, head + 256 + q_bytes, v.first);
    };
    return score_row_blocks(h, p, head_bytes, ws, ws_bytes, stream, filter, crng, seq.L - 1);
}
}  // extern "C++"

int sgpr_score_seq_positives(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols, int M,
                             int ctx, int L, int flags, int row0, const double* d_pose_xz, double d_pos, double d_neg,
                             const signed char* d_gt, int64_t ldg, float* d_out, int64_t capacity,
                             unsigned long long* d_count, void* d_workspace, size_t workspace_bytes, void* stream) {
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const PairTruth truth = eval_truth(row0, d_pose_xz, d_pos, d_neg, d_gt, ldg);
    if (!seq_eval_args_ok("sgpr_score_seq_positives", h, rect, ctx, L, flags, truth)) return SGPR_E_INVALID;
    if (!d_count || capacity < 0 || (capacity > 0 && !d_out)) {
        set_error("sgpr_score_seq_positives: NULL count buffer or capacity without an output buffer");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_seq_positives", sgpr_score_seq_positives_workspace_bytes(h, R, M, ctx, L, flags),
                      d_workspace, workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_score_seq_positives: memset");
    if (R == ctx || M == 0) return SGPR_OK;
    float* out = capacity > 0 ? d_out : nullptr;
    auto count = [&](const ScoreBlock& q, unsigned char*, int first) {
        return launch_pair_positives_more(h, q.score, q.R, M, M, truth_from(truth, first, first - ctx), out, capacity,
                                          d_count, s);
    };
    return seq_eval_blocks(h, rect, seq_spec(ctx, L, flags), seq_eval_head_bytes(R, M, L), d_workspace, workspace_bytes,
                           stream, count);
}

int sgpr_score_seq_threshold_counts(const sgpr_handle* h, const float* d_pooled_rows, int R, const float* d_pooled_cols,
                                    int M, int ctx, int L, int flags, int row0, const double* d_pose_xz, double d_pos,
                                    double d_neg, const signed char* d_gt, int64_t ldg, const float* d_thresholds, int T,
                                    const sgpr_rank_group* d_rank, int groups_per_threshold,
                                    const unsigned long long* d_at_least, unsigned long long* d_out, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
    const PooledRect rect = {d_pooled_rows, R, d_pooled_cols, M};
    const PairTruth truth = eval_truth(row0, d_pose_xz, d_pos, d_neg, d_gt, ldg);
    if (!seq_eval_args_ok("sgpr_score_seq_threshold_counts", h, rect, ctx, L, flags, truth)) return SGPR_E_INVALID;
    if (!d_out || T < 0 || T > SGPR_SCORE_COUNT_MAX_THRESHOLDS || (T > 0 && !d_thresholds)) {
        set_error("sgpr_score_seq_threshold_counts: 0.." + std::to_string(SGPR_SCORE_COUNT_MAX_THRESHOLDS) +
                  " thresholds and an output buffer");
        return SGPR_E_INVALID;
    }
    if (d_rank && (T < 1 || groups_per_threshold < 1 || !d_at_least)) {
        set_error("sgpr_score_seq_threshold_counts: the ranking needs thresholds, >= 1 value group per threshold and the pair counts");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok("sgpr_score_seq_threshold_counts",
                      sgpr_score_seq_threshold_counts_workspace_bytes(h, R, M, ctx, L, flags, T), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(d_out, 0, (size_t)(T + 3) * sizeof(unsigned long long), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_score_seq_threshold_counts: memset");
    if (R == ctx || M == 0) return SGPR_OK;
    auto count = [&](const ScoreBlock& q, unsigned char* tail, int first) {
        return launch_pair_counts_more(h, q.score, q.R, M, M, truth_from(truth, first, first - ctx), d_thresholds, T, d_rank,
                                       groups_per_threshold, d_at_least, d_out, reinterpret_cast<unsigned*>(tail), 1, s);
    };
    return seq_eval_blocks(h, rect, seq_spec(ctx, L, flags), seq_eval_head_bytes(R, M, L) + counts_head_bytes(h, T),
                           d_workspace, workspace_bytes, stream, count);
}

size_t sgpr_score_all_pairs_multi_workspace_bytes(const sgpr_handle* h, int n_jobs, const sgpr_pairs_job* jobs) {
    if (check_jobs(h, n_jobs, jobs) != SGPR_OK) return 0;
    size_t any = 0;
    if (h->generic_only && h->wm.ok)
        for (int j = 0; j < n_jobs; ++j) any = std::max(any, wide_tail_ws_bytes(jobs[j].R, jobs[j].M));
    return std::max(any, score_all_pairs_multi_ws_bytes(n_jobs, jobs));
}

int sgpr_score_all_pairs_multi(const sgpr_handle* h, int n_jobs, const sgpr_pairs_job* jobs, void* d_workspace,
                               size_t workspace_bytes, void* stream) {
    int rc = check_jobs(h, n_jobs, jobs);
    if (rc != SGPR_OK) return rc;
    if (h->generic_only) {
        DeviceGuard guard(h->device);
        for (int j = 0; j < n_jobs && rc == SGPR_OK; ++j)
            if (jobs[j].R > 0 && jobs[j].M > 0)
                rc = score_rect_any_shape(h, jobs[j].d_pooled_rows, jobs[j].R, jobs[j].d_pooled_cols, jobs[j].M, jobs[j].d_score,
                                          jobs[j].ld, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));   // (stream order
                                                                                     // lets the jobs share one workspace)
        return rc;
    }
    if (!workspace_ok("sgpr_score_all_pairs_multi", score_all_pairs_multi_ws_bytes(n_jobs, jobs), d_workspace,
                      workspace_bytes))
        return SGPR_E_WORKSPACE;
    DeviceGuard guard(h->device);
    if (tail_wide(h)) {             // the three-plane instance has no multi-rectangle form: job by job, in stream order,
        unsigned char* ws = static_cast<unsigned char*>(d_workspace);    // each in its slice of the workspace - the bits
        for (int j = 0; j < n_jobs && rc == SGPR_OK; ++j) {              // of sgpr_score_all_pairs on every rectangle
            const sgpr_pairs_job& q = jobs[j];
            if (q.R == 0 || q.M == 0) continue;
            rc = launch_score_all_pairs(h, q.d_pooled_rows, q.R, q.d_pooled_cols, q.M, q.d_score, q.ld, ws,
                                        static_cast<hipStream_t>(stream), true);
            ws += (score_all_pairs_ws_bytes(q.R, q.M) + 255) & ~(size_t)255;
        }
        return rc;
    }
    return launch_score_all_pairs_multi(h, n_jobs, jobs, d_workspace, static_cast<hipStream_t>(stream));
}

// workspace of sgpr_forward_dense: pooled [2B][32] | embed workspace for 2B graphs
size_t sgpr_forward_workspace_bytes(const sgpr_handle* h, int B, int N, int k) {
    EmbedPlan p;
    if (!h || B < 0) return 0;
    if (needs_generic(h, N, k)) {
        if (!generic_nk_ok(N, k)) return 0;
        const size_t pooled = ((size_t)2 * B * pooled_width(h) * sizeof(float) + 255) / 256 * 256;
        return pooled + generic_embed_ws_bytes(h, 2 * B, N, k) + 256;
    }
    if (!make_embed_plan(N, 0, k, &p)) return 0;
    return (size_t)2 * B * kF3 * sizeof(float) + embed_ws_bytes(h, 2 * B, N);
}

// sgpr_forward_dense on the any-shape kernels: the two sides embed as one launch of 2B graphs (one launch per side when
// the attention buffers are separate), then one wave per pair
static int forward_dense_generic(const sgpr_handle* h, const float* f1, const float* f2, int B, int N, int k,
                                 float* d_score, float* d_att1, float* d_att2, void* d_workspace,
                                 size_t workspace_bytes, void* stream) {
    const size_t need = sgpr_forward_workspace_bytes(h, B, N, k);
    if (need == 0) {
        set_error("sgpr_forward_dense: node_num " + std::to_string(N) + " / K " + std::to_string(k) + " outside the any-shape "
                  "limits (node_num <= " + std::to_string(SGPR_GENERIC_MAX_NODES) + ", K <= min(node_num, " +
                  std::to_string(SGPR_GENERIC_MAX_K) + "))");
        return (N < 1 || N > SGPR_GENERIC_MAX_NODES) ? SGPR_E_NODES : SGPR_E_K;
    }
    if (!d_workspace || workspace_bytes < need) {
        set_error("sgpr_forward_dense: workspace of " + std::to_string(need) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    const int pw = pooled_width(h);
    float* pooled = static_cast<float*>(d_workspace);
    const size_t pooled_bytes = ((size_t)2 * B * pw * sizeof(float) + 255) / 256 * 256;
    void* ws = static_cast<char*>(d_workspace) + pooled_bytes;
    const size_t ws_bytes = workspace_bytes - pooled_bytes;
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.dense = f1;
    a.dense2 = f2;
    a.g_split = B;
    a.G = 2 * B;
    a.pooled = pooled;
    int rc;
    if ((d_att1 && d_att2 && d_att2 == d_att1 + (size_t)B * N) || (!d_att1 && !d_att2)) {
        a.att = d_att1;
        rc = embed_generic(h, a, N, k, ws, ws_bytes, stream);
    } else {
        EmbedArgs a1 = a, a2 = a;
        a1.dense2 = nullptr; a1.G = B; a1.att = d_att1;
        a2.dense = f2; a2.dense2 = nullptr; a2.G = B; a2.att = d_att2;
        a2.pooled = pooled + (size_t)B * pw;
        rc = embed_generic(h, a1, N, k, ws, ws_bytes, stream);
        if (rc == SGPR_OK) rc = embed_generic(h, a2, N, k, ws, ws_bytes, stream);
    }
    if (rc != SGPR_OK) return rc;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h->generic_only)
        return launch_score_generic(h, pooled, nullptr, pooled + (size_t)B * pw, nullptr, B, 0, d_score, 0, s);
    return launch_score_pairs(h, pooled, nullptr, pooled + (size_t)B * kF3, nullptr, B, d_score, s);
}

int sgpr_forward_dense(const sgpr_handle* h, const float* d_features_1, const float* d_features_2, int B, int N,
                       int k, float* d_score, float* d_att1, float* d_att2, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
    if (!h || !d_features_1 || !d_features_2 || !d_score || B < 0) {
        set_error("sgpr_forward_dense: NULL argument or negative batch");
        return SGPR_E_INVALID;
    }
    if (needs_generic(h, N, k))
        return forward_dense_generic(h, d_features_1, d_features_2, B, N, k, d_score, d_att1, d_att2, d_workspace,
                                     workspace_bytes, stream);
    EmbedPlan plan;
    int rc = check_nk(2 * B, N, k, 0, &plan, wide_range(h), !h->dbg_prof && !(h->dbg_skip & ~kProductionSkipBits));
    if (rc != SGPR_OK) return rc;
    const size_t need = sgpr_forward_workspace_bytes(h, B, N, k);
    if (!d_workspace || workspace_bytes < need) {
        set_error("sgpr_forward_dense: workspace of " + std::to_string(need) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    float* pooled = static_cast<float*>(d_workspace);
    // both sides in ONE launch of 2B workgroups: graphs [0,B) = side 1, [B,2B) = side 2
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.dense = d_features_1;
    a.dense2 = d_features_2;
    a.g_split = B;
    a.G = 2 * B;
    a.pooled = pooled;
    a.redo = reinterpret_cast<unsigned char*>(pooled + (size_t)2 * B * kF3);
    a.redo_count = embed_redo_count(a.redo, 2 * B);      // (the per-side launches below share the word: tokens differ)
    a.park_ws = reinterpret_cast<float*>(a.redo + embed_flag_bytes(2 * B));
    a.status = h->d_status;
    a.prof = h->dbg_prof;
    a.skip = h->dbg_skip;
    a.num_labels = h->dims.num_labels;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_att1 && d_att2 && d_att2 == d_att1 + (size_t)B * N) {
        a.att = d_att1;  // contiguous [2B, N] attention buffer
        rc = launch_embed(h, plan, a, s);
    } else if (!d_att1 && !d_att2) {
        rc = launch_embed(h, plan, a, s);
    } else {
        // separate attention buffers: one launch per side
        EmbedArgs a1 = a, a2 = a;
        a1.dense2 = nullptr; a1.G = B; a1.att = d_att1;
        a2.dense = d_features_2; a2.dense2 = nullptr; a2.G = B; a2.att = d_att2;
        a2.pooled = pooled + (size_t)B * kF3;
        a2.redo = a.redo + B;
        a2.park_ws = a.park_ws + (size_t)B * ((N + 15) / 16 * 16) * 32;
        rc = launch_embed(h, plan, a1, s);
        if (rc == SGPR_OK) rc = launch_embed(h, plan, a2, s);
    }
    if (rc != SGPR_OK) return rc;
    return launch_score_pairs(h, pooled, nullptr, pooled + (size_t)B * kF3, nullptr, B, d_score, s);
}

int sgpr_knn(const float* d_x, int B, int C, int N, int k, int64_t* d_idx, void* stream) {
    if (B < 0 || C < 1) {
        set_error("sgpr_knn: negative batch or no channels");
        return SGPR_E_INVALID;
    }
    if (N < 1 || N > SGPR_ANY_MAX_NODES) {
        set_error("sgpr_knn: N " + std::to_string(N) + " outside [1, " + std::to_string(SGPR_ANY_MAX_NODES) + "]");
        return SGPR_E_NODES;
    }
    if (k < 1 || k > SGPR_ANY_MAX_K || k > N) {
        set_error("sgpr_knn: K " + std::to_string(k) + " outside [1, min(N, " + std::to_string(SGPR_ANY_MAX_K) + ")]");
        return SGPR_E_K;
    }
    if (B > 0 && (!d_x || !d_idx)) {                            // an empty batch may come with NULL (torch's empty data_ptr)
        set_error("sgpr_knn: NULL argument");
        return SGPR_E_INVALID;
    }
    if (N > SGPR_MAX_NODES || k > SGPR_MAX_K)                    // beyond the LDS-resident kernel: one wave per row
        return launch_knn_any(d_x, B, C, N, k, d_idx, static_cast<hipStream_t>(stream));
    return launch_knn(d_x, B, C, N, k, d_idx, static_cast<hipStream_t>(stream));
}

int sgpr_graph_feature(const float* d_x, const int64_t* d_idx, int B, int C, int N, int k, float* d_out, void* stream) {
    if (B < 0 || C < 1 || N < 1 || k < 1 || (B > 0 && (!d_x || !d_idx || !d_out))) {
        set_error("sgpr_graph_feature: NULL argument or non-positive size");
        return SGPR_E_INVALID;
    }
    return launch_graph_feature(d_x, d_idx, B, C, N, k, d_out, static_cast<hipStream_t>(stream));
}

int sgpr_attention_pool(const float* d_weight, const float* d_emb, int B, int N, float* d_rep, float* d_att,
                        void* stream) {
    if (B < 0 || N < 1) {
        set_error("sgpr_attention_pool: negative batch or no nodes");
        return SGPR_E_INVALID;
    }
    if ((size_t)N * sizeof(float) > 48 * 1024) {
        set_error("sgpr_attention_pool: more than 12288 nodes per graph");
        return SGPR_E_NODES;
    }
    if (B > 0 && (!d_weight || !d_emb || !d_rep)) {
        set_error("sgpr_attention_pool: NULL argument");
        return SGPR_E_INVALID;
    }
    return launch_attention_pool(d_weight, d_emb, B, N, d_rep, d_att, static_cast<hipStream_t>(stream));
}

int sgpr_attention_pool_any(const float* d_weight, const float* d_emb, int B, int N, int F, float* d_rep, float* d_att,
                            void* stream) {
    if (B < 0 || N < 1) {
        set_error("sgpr_attention_pool_any: negative batch or no nodes");
        return SGPR_E_INVALID;
    }
    if (F < 1 || F > SGPR_ANY_MAX_FILTERS_3) {
        set_error("sgpr_attention_pool_any: width " + std::to_string(F) + " outside [1, " +
                  std::to_string(SGPR_ANY_MAX_FILTERS_3) + "]");
        return SGPR_E_DIMS;
    }
    if (B > 0 && (!d_weight || !d_emb || !d_rep)) {
        set_error("sgpr_attention_pool_any: NULL argument");
        return SGPR_E_INVALID;
    }
    return launch_attention_any(d_weight, d_emb, B, N, F, d_rep, d_att, static_cast<hipStream_t>(stream));
}

int sgpr_ntn_any(const float* d_weight, const float* d_weight_block, const float* d_bias, const float* d_e1,
                 const float* d_e2, int64_t B, int F, int T, float* d_out, void* stream) {
    if (B < 0) {
        set_error("sgpr_ntn_any: negative batch");
        return SGPR_E_INVALID;
    }
    if (F < 1 || F > SGPR_ANY_MAX_FILTERS_3 || T < 1 || T > SGPR_ANY_MAX_NEURONS) {
        set_error("sgpr_ntn_any: width " + std::to_string(F) + " / " + std::to_string(T) + " neurons outside [1, " +
                  std::to_string(SGPR_ANY_MAX_FILTERS_3) + "] / [1, " + std::to_string(SGPR_ANY_MAX_NEURONS) + "]");
        return SGPR_E_DIMS;
    }
    if (B > 0 && (!d_weight || !d_weight_block || !d_bias || !d_e1 || !d_e2 || !d_out)) {
        set_error("sgpr_ntn_any: NULL argument");
        return SGPR_E_INVALID;
    }
    return launch_ntn_any(d_weight, d_weight_block, d_bias, d_e1, d_e2, B, F, T, d_out, static_cast<hipStream_t>(stream));
}

int sgpr_ntn(const float* d_weight, const float* d_weight_block, const float* d_bias, const float* d_e1,
             const float* d_e2, int64_t B, float* d_out, void* stream) {
    if (B < 0 || (B > 0 && (!d_weight || !d_weight_block || !d_bias || !d_e1 || !d_e2 || !d_out))) {
        set_error("sgpr_ntn: NULL argument or negative batch");
        return SGPR_E_INVALID;
    }
    return launch_ntn(d_weight, d_weight_block, d_bias, d_e1, d_e2, B, d_out, static_cast<hipStream_t>(stream));
}

int sgpr_verify_pairs(const float* d_centers_a, const int32_t* d_labels_a, int GA, const float* d_centers_b,
                      const int32_t* d_labels_b, int GB, int N, const int32_t* d_idx_a, const int32_t* d_idx_b, int64_t P,
                      float tau_edge, float tau_in, float tau_z, float min_base, int max_hyp, sgpr_verify_result* d_out,
                      void* stream) {
    static_assert(sizeof(sgpr_verify_result) == 88, "sgpr_verify_result is 88 bytes without padding");
    if (P < 0 || GA < 0 || GB < 0) {
        set_error("sgpr_verify_pairs: negative count");
        return SGPR_E_INVALID;
    }
    // (a NaN fails every >= test)
    if (!(tau_edge >= 0.f) || !(tau_in >= 0.f) || !(tau_z >= 0.f) || !(min_base >= 0.f) || max_hyp < 1) {
        set_error("sgpr_verify_pairs: tolerances must be >= 0 and not NaN, max_hyp >= 1");
        return SGPR_E_INVALID;
    }
    if (N < 1 || N > SGPR_VERIFY_MAX_NODES) {
        set_error("sgpr_verify_pairs: N " + std::to_string(N) + " outside [1, " + std::to_string(SGPR_VERIFY_MAX_NODES) + "]");
        return SGPR_E_NODES;
    }
    // (an empty list may come with NULL: the data pointer of an empty torch tensor)
    if (P > 0 && (!d_idx_a || !d_idx_b || !d_out || !d_centers_a || !d_labels_a || !d_centers_b || !d_labels_b)) {
        set_error("sgpr_verify_pairs: NULL argument");
        return SGPR_E_INVALID;
    }
    if (P == 0) return SGPR_OK;
    return launch_verify_pairs(d_centers_a, d_labels_a, GA, d_centers_b, d_labels_b, GB, N, d_idx_a, d_idx_b, P, tau_edge,
                               tau_in, tau_z, min_base, max_hyp, d_out, static_cast<hipStream_t>(stream));
}

static bool consistency_counts_ok(const char* fn, int C, int n_groups) {
    if (C < 0 || C > SGPR_CONSISTENCY_MAX_CLOSURES) {
        set_error(std::string(fn) + ": C " + std::to_string(C) + " outside [0, " +
                  std::to_string(SGPR_CONSISTENCY_MAX_CLOSURES) + "]");
        return false;
    }
    if (n_groups < 1 || n_groups > SGPR_CONSISTENCY_MAX_GROUPS) {
        set_error(std::string(fn) + ": n_groups " + std::to_string(n_groups) + " outside [1, " +
                  std::to_string(SGPR_CONSISTENCY_MAX_GROUPS) + "]");
        return false;
    }
    return true;
}

size_t sgpr_closure_consistency_workspace_bytes(int C) {
    return (C < 0 || C > SGPR_CONSISTENCY_MAX_CLOSURES) ? 0 : closure_consistency_ws_bytes(C);
}

size_t sgpr_consistent_set_workspace_bytes(int C) {
    return (C < 0 || C > SGPR_CONSISTENCY_MAX_CLOSURES) ? 0 : consistent_set_ws_bytes(C);
}

int sgpr_closure_consistency(const int32_t* d_rows, const int32_t* d_cols, const double* d_T, int C, const double* d_Xr,
                             int MR, const double* d_Xc, int MC, const int32_t* d_group, int n_groups, double max_trans,
                             double min_cos, double lever_gain, uint64_t* d_adj, int32_t* d_degree, void* d_workspace,
                             size_t workspace_bytes, void* stream) {
    if (!consistency_counts_ok("sgpr_closure_consistency", C, n_groups)) return SGPR_E_INVALID;
    if (MR < 0 || MC < 0) {
        set_error("sgpr_closure_consistency: negative pose table size");
        return SGPR_E_INVALID;
    }
    // (a NaN fails every comparison)
    if (!(max_trans >= 0.0) || !(lever_gain >= 0.0)) {
        set_error("sgpr_closure_consistency: max_trans and lever_gain must be >= 0 and not NaN");
        return SGPR_E_INVALID;
    }
    if (min_cos != min_cos) {
        set_error("sgpr_closure_consistency: min_cos is NaN");
        return SGPR_E_INVALID;
    }
    if (C == 0) return SGPR_OK;
    // (an empty pose table may come with NULL: every closure is then void)
    if (!d_rows || !d_cols || !d_T || !d_group || !d_adj || !d_degree || (MR > 0 && !d_Xr) || (MC > 0 && !d_Xc)) {
        set_error("sgpr_closure_consistency: NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = closure_consistency_ws_bytes(C);
    if (!d_workspace || workspace_bytes < need) {
        set_error("sgpr_closure_consistency: workspace of " + std::to_string(need) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    return launch_closure_consistency(d_rows, d_cols, d_T, C, d_Xr, MR, d_Xc, MC, d_group, n_groups, max_trans, min_cos,
                                      lever_gain, reinterpret_cast<unsigned long long*>(d_adj), d_degree, d_workspace,
                                      static_cast<hipStream_t>(stream));
}

int sgpr_consistent_set(const uint64_t* d_adj, int C, const int32_t* d_group, int n_groups, int32_t* d_rank,
                        int32_t* d_group_size, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!consistency_counts_ok("sgpr_consistent_set", C, n_groups)) return SGPR_E_INVALID;
    if (C == 0) {
        if (d_group_size) {
            const hipError_t e = hipMemsetAsync(d_group_size, 0, (size_t)n_groups * sizeof(int32_t),
                                                static_cast<hipStream_t>(stream));
            if (e != hipSuccess) return hip_fail(e, "sgpr_consistent_set: clearing d_group_size");
        }
        return SGPR_OK;
    }
    if (!d_adj || !d_group || !d_rank || !d_group_size) {
        set_error("sgpr_consistent_set: NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = consistent_set_ws_bytes(C);
    if (!d_workspace || workspace_bytes < need) {
        set_error("sgpr_consistent_set: workspace of " + std::to_string(need) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    return launch_consistent_set(reinterpret_cast<const unsigned long long*>(d_adj), C, d_group, n_groups, d_rank,
                                 d_group_size, d_workspace, static_cast<hipStream_t>(stream));
}

size_t sgpr_cluster_workspace_bytes(int P) { return P < 0 ? 0 : cluster_ws_bytes(P); }

int sgpr_cluster_scan(const float* d_points, int point_stride, const uint32_t* d_labels, int P, int max_nodes,
                      double* d_centers, int32_t* d_node_labels, int32_t* d_node_sizes, int32_t* d_point_node,
                      int32_t* d_num_nodes, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || max_nodes < 0 || point_stride < 3 || !d_num_nodes || (P > 0 && (!d_points || !d_labels)) ||
        (max_nodes > 0 && (!d_centers || !d_node_labels || !d_node_sizes))) {
        set_error("sgpr_cluster_scan: NULL argument, negative count or point_stride < 3");
        return SGPR_E_INVALID;
    }
    const size_t need = cluster_ws_bytes(P);
    if (!d_workspace || workspace_bytes < need) {
        set_error("sgpr_cluster_scan: workspace of " + std::to_string(need) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    return launch_cluster_scan(d_points, point_stride, d_labels, P, max_nodes, d_centers, d_node_labels, d_node_sizes,
                               d_point_node, d_num_nodes, d_workspace, static_cast<hipStream_t>(stream));
}

int sgpr_graph_edges(const float* d_points, int point_stride, const int32_t* d_point_node, int P, int n,
                     const double* d_centers, double* d_min_dis, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || n < 0 || n > 8192 || point_stride < 3 || (n > 0 && (!d_points || !d_point_node || !d_centers || !d_min_dis))) {
        set_error("sgpr_graph_edges: NULL argument, negative count or point_stride < 3");
        return SGPR_E_INVALID;
    }
    if (n > 0 && (!d_workspace || workspace_bytes < (size_t)n * n * sizeof(int))) {
        set_error("sgpr_graph_edges: workspace of " + std::to_string((size_t)n * n * sizeof(int)) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    return launch_graph_edges(d_points, point_stride, d_point_node, P, n, d_centers, d_min_dis, d_workspace,
                              static_cast<hipStream_t>(stream));
}

void sgpr_debug_set_skip_mask(sgpr_handle* h, int mask) {
    if (h) h->dbg_skip = mask;
}

int sgpr_debug_uses_f16_planes(const sgpr_handle* h) { return (h && h->f16_weights) ? 1 : 0; }

void sgpr_debug_set_profile_buffer(sgpr_handle* h, void* d_counters) {
    if (h) h->dbg_prof = static_cast<unsigned long long*>(d_counters);
}

int sgpr_check_status(const sgpr_handle* h, void* stream) {
    if (!h) {
        set_error("sgpr_check_status: NULL handle");
        return SGPR_E_INVALID;
    }
    int32_t flag = 0;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(&flag, h->d_status, sizeof(flag), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_check_status");
    if (flag) {
        e = hipMemsetAsync(h->d_status, 0, sizeof(flag), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "sgpr_check_status: reset");
        if (flag & 32) {
            set_error("internal: the second pass of sgpr_score_above / sgpr_rows_above wrote a different number of pairs "
                      "than its first pass counted");
            return SGPR_E_HIP;
        }
        if (flag & 16) {
            set_error("a d_row_self entry of sgpr_score_topk / sgpr_score_above / sgpr_score_mine lies outside [0, M)");
            return SGPR_E_INVALID;
        }
        if (flag & 4) {
            set_error("internal: a semantic wave of the split embed launch did not deliver (pooled vector set to NaN)");
            return SGPR_E_HIP;
        }
        if (flag & 8) {
            set_error("a graph of the ragged store holds more nodes than node_num slots, or its offsets decrease (its pooled vector is NaN)");
            return SGPR_E_NODES;
        }
        if (flag & 2) {
            set_error("a graph needed more slots than the node_cap passed to sgpr_embed_capped (its pooled vector is NaN)");
            return SGPR_E_NODES;
        }
        set_error("a node label outside [-1, num_labels) was seen by the embed kernel");
        return SGPR_E_LABEL;
    }
    return SGPR_OK;
}

}  // extern "C"

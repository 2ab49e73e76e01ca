// Host-only model packer: one checkpoint blob -> one BatchNorm fold (FoldedNet) -> the three device layouts
// (DevWeights / GenericModel / WideModel of sgpr_internal.hpp) as host buffers + offsets.  Plain C++17, no HIP: what
// sgpr_create uploads is exactly what these functions return, so the layouts are testable without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "sgpr.h"

namespace sgpr {

// Architecture the kernels are written for (every shipped checkpoint; sgpr.h).
constexpr int kLabels = 12;
constexpr int kF1 = 64, kF2 = 64, kF3 = 32;
constexpr int kT = 16;   // tensor_neurons
constexpr int kB = 16;   // bottle_neck_neurons
constexpr int kKPad = 16;  // layer-1 inputs (3 / 12 channels) are zero-padded to one MFMA k-block

constexpr int kSemTableFloats = 4 * 256 + 32 + 2 * 2 * 16 * 64;

// Any-shape model (sgpr_generic.hip): the folded fp32 weights at the model's own dimensions, for what the tuned kernels
// are not built for - architectures beyond the built shape, node_num > SGPR_MAX_NODES, K > SGPR_MAX_K.
#define SGPR_GENERIC_MAX_LABELS SGPR_ANY_MAX_LABELS
#define SGPR_GENERIC_MAX_FILTERS SGPR_ANY_MAX_FILTERS
#define SGPR_GENERIC_MAX_F3 SGPR_ANY_MAX_FILTERS_3
#define SGPR_GENERIC_MAX_T SGPR_ANY_MAX_NEURONS          // tensor neurons and bottleneck neurons
#define SGPR_GENERIC_MAX_NODES SGPR_ANY_MAX_NODES
#define SGPR_GENERIC_MAX_K SGPR_ANY_MAX_K

// Limits of the matrix-core form of the any-shape model (WideModel, sgpr_wide.hip)
#define SGPR_WIDE_MAX_LABELS 32
#define SGPR_WIDE_MAX_FILTERS 128
#define SGPR_WIDE_MAX_F3 64
#define SGPR_WIDE_MAX_NODES 112
#ifndef SGPR_WIDE_EMBED
#define SGPR_WIDE_EMBED 1     // any-shape handles inside sgpr_wide.hip's limits embed on the matrix cores (0: A/B builds, plain fp32 only)
#endif

// The kernels are written for {12, 64, 64, 32, 16, 16}.  A SMALLER architecture is served exactly by the same kernels:
// its tensors are embedded into the built shapes with zero weights for the channels it does not have - a channel whose
// weights are all zero stays 0 through conv / BN / LeakyReLU, adds 0 to every distance, every sum and every maximum
// partner, and a zero tensor / bottleneck neuron contributes 0 to the score.
inline bool dims_supported(const sgpr_dims* d) {
    return d && d->num_labels >= 1 && d->num_labels <= kLabels && d->filters_1 >= 1 && d->filters_1 <= kF1 &&
           d->filters_2 >= 1 && d->filters_2 <= kF2 && d->filters_3 >= 1 && d->filters_3 <= kF3 &&
           d->tensor_neurons >= 1 && d->tensor_neurons <= kT && d->bottle_neck_neurons >= 1 && d->bottle_neck_neurons <= kB;
}

// what the any-shape kernels (sgpr_generic.hip) serve
inline bool dims_generic(const sgpr_dims* d) {
    return d && d->num_labels >= 1 && d->num_labels <= SGPR_GENERIC_MAX_LABELS && d->filters_1 >= 1 &&
           d->filters_1 <= SGPR_GENERIC_MAX_FILTERS && d->filters_2 >= 1 && d->filters_2 <= SGPR_GENERIC_MAX_FILTERS &&
           d->filters_3 >= 1 && d->filters_3 <= SGPR_GENERIC_MAX_F3 && d->tensor_neurons >= 1 &&
           d->tensor_neurons <= SGPR_GENERIC_MAX_T && d->bottle_neck_neurons >= 1 && d->bottle_neck_neurons <= SGPR_GENERIC_MAX_T;
}

struct BlockShape {
    int cout, cin2;
};

inline void block_shapes(const sgpr_dims* d, BlockShape out[7]) {
    // order of the blob: s_conv1, f_conv1, s_conv2, f_conv2, s_conv3, f_conv3, conv_end (sg_net.py:50-76)
    out[0] = {d->filters_1, 6};
    out[1] = {d->filters_1, 2 * d->num_labels};
    out[2] = {d->filters_2, 2 * d->filters_1};
    out[3] = {d->filters_2, 2 * d->filters_1};
    out[4] = {d->filters_3, 2 * d->filters_2};
    out[5] = {d->filters_3, 2 * d->filters_2};
    out[6] = {d->filters_3, 2 * d->filters_3};
}

// The eight tensors behind the convolution blocks, in blob order, each as [s0][s1][s2]
enum Tail { kAttW, kNtnW, kNtnWb, kNtnBias, kFc1W, kFc1B, kFc2W, kFc2B, kTails };
struct TailShape {
    size_t s[3];
    size_t count() const { return s[0] * s[1] * s[2]; }
};
inline void tail_shapes(const sgpr_dims* d, TailShape out[kTails]) {
    const size_t f = d->filters_3, t = d->tensor_neurons, bn = d->bottle_neck_neurons;
    out[kAttW] = {{f, f, 1}};        // attention.weight_matrix [F3][F3]
    out[kNtnW] = {{f, f, t}};        // tensor_network.weight_matrix [F3][F3][T]
    out[kNtnWb] = {{t, 2, f}};       // tensor_network.weight_matrix_block [T][2 F3]: the two halves keep their places
    out[kNtnBias] = {{t, 1, 1}};     // tensor_network.bias [T]
    out[kFc1W] = {{bn, t, 1}};       // fully_connected_first.weight [B][T]
    out[kFc1B] = {{bn, 1, 1}};       // fully_connected_first.bias [B]
    out[kFc2W] = {{bn, 1, 1}};       // scoring_layer.weight [1][B]
    out[kFc2B] = {{1, 1, 1}};        // scoring_layer.bias
}

inline size_t weights_count(const sgpr_dims* d) {
    BlockShape bs[7];
    block_shapes(d, bs);
    TailShape ts[kTails];
    tail_shapes(d, ts);
    size_t n = 0;
    for (int b = 0; b < 7; ++b) n += (size_t)bs[b].cout * bs[b].cin2 + 4 * (size_t)bs[b].cout;
    for (int q = 0; q < kTails; ++q) n += ts[q].count();
    return n;
}

// The scoring head's fold v[o][t] = fc2_w[o] fc1_w[o][t] (fp32, as every tail forms it) is cut into two f16 planes by
// the matrix-core tails.  A plane pair keeps 22 significant bits only where the low plane is normal (|v| >= 2^-3); below
// that the low plane's step is a fixed 2^-24.  The tails therefore cut 2^k v, k >= 0 the largest power that keeps
// max |2^k v| below 2^15 (k <= 64), scale b1 by the same factor and undo it in the sigmoid's constant: exp2(z' (-log2 e
// 2^-k) + ...) with z' = 2^k z is the unscaled product exactly.  f16_ok = 0: max |v| reaches 60000, no f16 plane can hold
// the fold and the handle's tails run at fp32's range (the bf16 instance / the plain-fp32 kernel).
struct HeadRange {
    float scale, nl2e;
    int f16_ok;
};
inline HeadRange head_range(const float* fc1_w, const float* fc2_w, int B, int T) {
    float vmax = 0.f;
    bool finite = true;
    for (int o = 0; o < B; ++o)
        for (int t = 0; t < T; ++t) {
            const float v = fabsf(fc2_w[o] * fc1_w[(size_t)o * T + t]);
            if (!(v <= 3.0e38f)) finite = false;
            vmax = v > vmax ? v : vmax;
        }
    HeadRange r;
    r.f16_ok = finite && vmax < 60000.f;
    int k = 0;
    if (r.f16_ok && vmax > 0.f)
        while (k < 64 && ldexpf(vmax, k + 1) < 32768.f) ++k;
    r.scale = ldexpf(1.f, k);
    r.nl2e = ldexpf(-1.4426950408889634f, -k);
    return r;
}

// w = hi + mid + lo with three round-to-nearest-even bf16 terms (exact to 24 bits)
inline unsigned short bf16_rne_host(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
inline float bf16_to_float_host(unsigned short h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline void split3_host(float w, unsigned short* pl) {
    pl[0] = bf16_rne_host(w);
    float r = w - bf16_to_float_host(pl[0]);
    pl[1] = bf16_rne_host(r);
    r -= bf16_to_float_host(pl[1]);
    pl[2] = bf16_rne_host(r);
}
// w = hi + lo with two f16 terms (22 bits)
inline void split2_host(float w, unsigned short* pl) {
    const _Float16 hi = (_Float16)w;
    const _Float16 lo = (_Float16)(w - (float)hi);
    memcpy(&pl[0], &hi, 2);
    memcpy(&pl[1], &lo, 2);
}

// ---- the one BatchNorm fold: eval-mode statistics folded into the 1x1 convolutions in double precision, at the
//      checkpoint's own dimensions.  Blob order: s_conv1, f_conv1, s_conv2, f_conv2, s_conv3, f_conv3, conv_end.
struct FoldedBlock {
    int cout, cols;             // cols: cin of an EdgeConv block (a and b), 2 cin of conv_end (a alone)
    std::vector<float> a;       // [cout][cols]  s * W[:, :cin]   (acts on x_j; dgcnn.py:47)   conv_end: s * W
    std::vector<float> b;       // [cout][cols]  s * (W[:, cin:] - W[:, :cin])   (acts on x_i)
    std::vector<float> t;       // [cout]        beta - mean * s,  s = gamma / sqrt(var + 1e-5)
    std::vector<float> z;       // [cout]        s * 0: what the fold makes of a zero weight (-0 under a negative gamma) -
                                //               the built shape's padded INPUT channels of a real output channel
};
struct FoldedNet {
    sgpr_dims dims;
    FoldedBlock blk[7];
    const float* tail[kTails];  // views into the caller's blob
    TailShape ts[kTails];
};

inline FoldedNet fold_model(const float* weights, const sgpr_dims* d) {
    FoldedNet n;
    n.dims = *d;
    BlockShape bs[7];
    block_shapes(d, bs);
    const float* src = weights;
    for (int b = 0; b < 7; ++b) {
        const int cout = bs[b].cout, cin2 = bs[b].cin2;
        const bool edge = b < 6;
        const int cols = edge ? cin2 / 2 : cin2;
        const float* W = src;
        const float* gamma = W + (size_t)cout * cin2;
        const float* beta = gamma + cout;
        const float* mean = beta + cout;
        const float* var = mean + cout;
        src = var + cout;
        FoldedBlock& k = n.blk[b];
        k.cout = cout;
        k.cols = cols;
        k.a.resize((size_t)cout * cols);
        k.b.resize(edge ? (size_t)cout * cols : 0);
        k.t.resize(cout);
        k.z.resize(cout);
        for (int c = 0; c < cout; ++c) {
            const double s = (double)gamma[c] / sqrt((double)var[c] + 1e-5);
            for (int i = 0; i < cols; ++i) {
                const double w1 = W[(size_t)c * cin2 + i];
                k.a[(size_t)c * cols + i] = (float)(s * w1);
                if (edge) {
                    const double w2 = W[(size_t)c * cin2 + cols + i];
                    k.b[(size_t)c * cols + i] = (float)(s * (w2 - w1));
                }
            }
            k.t[c] = (float)((double)beta[c] - (double)mean[c] * s);
            k.z[c] = (float)(s * 0.0);
        }
    }
    tail_shapes(d, n.ts);
    for (int q = 0; q < kTails; ++q) {
        n.tail[q] = src;
        src += n.ts[q].count();
    }
    return n;
}

// ---- the one MFMA operand order: [column tile][k-step][plane][lane][8].  Lane = 16*lq + l15 holds row ct*16 + l15 and
//      k = 32*step + 8*lq + 0..7; first layers (k16, K = 16): one step, k = 4*lq + 0..3 then four zeros.
//      value(row, k) is the matrix (0 outside it), split(v, pl) cuts a value into PLANES terms.
template <int PLANES, class Value, class Split>
inline std::vector<unsigned short> pack_fragments(int nct, int nks, bool k16, Value value, Split split) {
    std::vector<unsigned short> out((size_t)nct * nks * PLANES * 512, 0);
    for (int ct = 0; ct < nct; ++ct)
        for (int st = 0; st < nks; ++st)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int row = ct * 16 + (lane & 15), lq = lane >> 4;
                    const int k = k16 ? (j < 4 ? 4 * lq + j : -1) : 32 * st + 8 * lq + j;
                    unsigned short pl[PLANES] = {};
                    if (k >= 0) split(value(row, k), pl);
                    for (int q = 0; q < PLANES; ++q) out[(((size_t)(ct * nks + st) * PLANES + q) * 64 + lane) * 8 + j] = pl[q];
                }
    return out;
}

// ---- DevWeights: the built shape {12, 64, 64, 32, 16, 16}, a smaller checkpoint scattered into it with zero fill
struct PackedBuilt {
    std::vector<float> blob;            // one allocation; every offset below is a float index into it
    // EdgeConv layers in KERNEL order f1,f2,f3,s1,s2,s3 (the semantic branch runs first: its 12 input registers per
    // thread die after the first staging, the 3 xyz registers wait for the second); [6] is conv_end
    size_t off_wf[7], off_tb[7], off_wb[7], off_wh[7];
    int kp[6], cout[6];
    size_t off_tail[kTails];
    size_t off_ntwt;                    // NTN weight re-ordered [i][t][j] for the all-pairs prep kernel
    size_t off_semtab;                  // kSemTableFloats + 4 zeros: sgpr_create fills them on the device
    bool f16_ok;                        // every folded convolution weight fits the f16 range
    HeadRange head;
};

inline PackedBuilt pack_built(const FoldedNet& n) {
    const sgpr_dims full = {kLabels, kF1, kF2, kF3, kT, kB};
    BlockShape bf[7];
    block_shapes(&full, bf);
    PackedBuilt out;
    std::vector<float>& p = out.blob;
    size_t off_wf[7], off_tb[7], off_wb[7], off_wh[7];      // blob order
    int kp_of[7], rows_of[7];
    for (int b = 0; b < 7; ++b) {
        const FoldedBlock& k = n.blk[b];
        const bool edge = b < 6;
        const int CO = bf[b].cout, cols = edge ? bf[b].cin2 / 2 : bf[b].cin2;
        const int kp = edge && cols <= kKPad ? kKPad : cols;
        kp_of[b] = kp;
        rows_of[b] = edge ? 2 * CO : CO;
        off_wf[b] = p.size();
        p.resize(p.size() + (size_t)rows_of[b] * kp, 0.f);
        float* wf = p.data() + off_wf[b];
        for (int c = 0; c < k.cout; ++c)
            for (int i = 0; i < cols; ++i) {
                // the checkpoint's column behind built column i: an EdgeConv half keeps its place in the wider half,
                // conv_end keeps the xyz3 half and the sem3 half of cat(xyz3, sem3)
                const int half = edge ? 0 : i / kF3, r = edge ? i : i % kF3, width = edge ? k.cols : k.cols / 2;
                const bool real = r < width;
                const size_t at = (size_t)c * k.cols + half * width + r;
                wf[(size_t)c * kp + i] = real ? k.a[at] : k.z[c];
                if (edge) wf[(size_t)(CO + c) * kp + i] = real ? k.b[at] : k.z[c];
            }
        off_tb[b] = p.size();
        p.resize(p.size() + CO, 0.f);
        std::copy(k.t.begin(), k.t.end(), p.begin() + off_tb[b]);
    }
    TailShape tf[kTails];
    tail_shapes(&full, tf);
    for (int q = 0; q < kTails; ++q) {
        const TailShape& u = n.ts[q];
        out.off_tail[q] = p.size();
        p.resize(p.size() + tf[q].count(), 0.f);
        float* dst = p.data() + out.off_tail[q];
        for (size_t i = 0; i < u.s[0]; ++i)
            for (size_t j = 0; j < u.s[1]; ++j)
                for (size_t l = 0; l < u.s[2]; ++l)
                    dst[(i * tf[q].s[1] + j) * tf[q].s[2] + l] = n.tail[q][(i * u.s[1] + j) * u.s[2] + l];
    }
    const size_t f = kF3, t = kT;
    while (p.size() % 4) p.push_back(0.f);
    out.off_ntwt = p.size();
    p.resize(p.size() + f * f * t);
    for (size_t i = 0; i < f; ++i)
        for (size_t tt = 0; tt < t; ++tt)
            for (size_t j = 0; j < f; ++j) p[out.off_ntwt + (i * t + tt) * f + j] = p[out.off_tail[kNtnW] + i * (f * t) + j * t + tt];
    auto append = [&p](const std::vector<unsigned short>& planes) {
        const size_t at = p.size();
        p.resize(at + planes.size() / 2);
        memcpy(p.data() + at, planes.data(), planes.size() * sizeof(unsigned short));
        return at;
    };
    // the seven folded matrices as three bf16 planes, then as two f16 planes (the default), in MFMA operand order
    out.f16_ok = true;
    for (int planes = 3; planes >= 2; --planes)
        for (int b = 0; b < 7; ++b) {
            const int kp = kp_of[b], nks = kp == 64 ? 2 : 1, nct = rows_of[b] / 16;
            const size_t wf = off_wf[b];
            auto value = [&p, wf, kp](int row, int k) { return p[wf + (size_t)row * kp + k]; };
            if (planes == 3)
                off_wb[b] = append(pack_fragments<3>(nct, nks, nks == 1, value, split3_host));
            else
                off_wh[b] = append(pack_fragments<2>(nct, nks, nks == 1, value, [&out](float v, unsigned short* pl) {
                    if (!(fabsf(v) < 60000.f)) out.f16_ok = false;
                    split2_host(v, pl);
                }));
        }
    while (p.size() % 4) p.push_back(0.f);
    out.off_semtab = p.size();          // graph-independent tables of the super-node branch + the largest value in them
    p.resize(p.size() + kSemTableFloats + 4, 0.f);

    static const int blob_of_layer[7] = {1, 3, 5, 0, 2, 4, 6};      // blob order is s1,f1,s2,f2,s3,f3
    for (int l = 0; l < 7; ++l) {
        const int b = blob_of_layer[l];
        out.off_wf[l] = off_wf[b];
        out.off_tb[l] = off_tb[b];
        out.off_wb[l] = off_wb[b];
        out.off_wh[l] = off_wh[b];
        if (l < 6) {
            out.kp[l] = kp_of[b];
            out.cout[l] = bf[b].cout;
        }
    }
    out.head = head_range(p.data() + out.off_tail[kFc1W], p.data() + out.off_tail[kFc2W], kB, kT);
    return out;
}

// ---- GenericModel: fp32 at the checkpoint's own dimensions, one allocation
struct PackedGeneric {
    std::vector<float> blob;
    int cin[6], cout[6], cmax;          // EdgeConv blocks: xyz branch (s_conv1..3), then the semantic branch (f_conv1..3)
    size_t off_wa[6], off_wb[6], off_tb[6], off_wend, off_tend;
    size_t off_tail[kTails];
    HeadRange head;
};

inline PackedGeneric pack_generic(const FoldedNet& n) {
    PackedGeneric out;
    std::vector<float>& host = out.blob;
    const sgpr_dims& d = n.dims;
    out.cmax = std::max(std::max(3, d.num_labels), std::max(d.filters_1, std::max(d.filters_2, d.filters_3)));
    // [cols][cout8]: input-channel-major, the output channels padded to a multiple of 8 (see GenericModel)
    auto put = [&host](const std::vector<float>& m, int cout, int cols) {
        const int cout8 = (cout + 7) & ~7;
        const size_t at = host.size();
        host.resize(at + (size_t)cout8 * cols, 0.f);
        for (int c = 0; c < cout; ++c)
            for (int i = 0; i < cols; ++i) host[at + (size_t)i * cout8 + c] = m[(size_t)c * cols + i];
        return at;
    };
    for (int b = 0; b < 7; ++b) {
        const FoldedBlock& k = n.blk[b];
        if (b < 6) {
            // blob order alternates the branches (s1, f1, s2, f2, s3, f3); the model keeps xyz layers 0..2, semantic 3..5
            const int l6 = (b & 1) * 3 + (b >> 1);
            out.cin[l6] = k.cols;
            out.cout[l6] = k.cout;
            out.off_wa[l6] = put(k.a, k.cout, k.cols);
            out.off_wb[l6] = put(k.b, k.cout, k.cols);
            out.off_tb[l6] = put(k.t, k.cout, 1);
        } else {
            out.off_wend = put(k.a, k.cout, k.cols);
            out.off_tend = put(k.t, k.cout, 1);
        }
    }
    for (int q = 0; q < kTails; ++q) {
        out.off_tail[q] = host.size();
        host.insert(host.end(), n.tail[q], n.tail[q] + n.ts[q].count());
    }
    out.head = head_range(n.tail[kFc1W], n.tail[kFc2W], d.bottle_neck_neurons, d.tensor_neurons);
    return out;
}

// ---- WideModel: the matrix-core form of the same folded weights (sgpr_wide.hip) for moderately larger architectures:
//      widths padded to 32 with zeros, two f16 planes (w = hi + lo, 22 bits) in MFMA operand order.  Only for an
//      any-shape handle (the built shape runs on the tuned kernels) inside the limits and the f16 range.
struct PackedWide {
    bool ok;                            // false: not served, no buffer
    std::vector<unsigned short> planes;
    std::vector<float> tbs;
    size_t plane_bytes;                 // the biases follow the planes at this byte offset of the allocation
    int cinP[6], coutP[6], F3P;         // GenericModel's layer order
    size_t off_wh[7], off_tbp[7];       // [6]: conv_end
};

inline PackedWide pack_wide(const FoldedNet& n, bool generic_only) {
    PackedWide out = {};                // (ok = false, every scalar 0)
    const sgpr_dims& d = n.dims;
    float wmax = 0.f;
    for (int b = 0; b < 7; ++b)
        for (const std::vector<float>* m : {&n.blk[b].a, &n.blk[b].b, &n.blk[b].t})
            for (float v : *m) wmax = std::max(wmax, fabsf(v));
    // (the head fold fc2_w * fc1_w the wide tail cuts into f16 planes is not range-checked here: see ADVICE.md)
    if (!(generic_only && d.num_labels <= SGPR_WIDE_MAX_LABELS && d.filters_1 <= SGPR_WIDE_MAX_FILTERS &&
          d.filters_2 <= SGPR_WIDE_MAX_FILTERS && d.filters_3 <= SGPR_WIDE_MAX_F3 && wmax < 60000.f && SGPR_WIDE_EMBED))
        return out;
    out.ok = true;
    auto p32 = [](int v) { return (v + 31) & ~31; };
    auto append = [&out](int l, const std::vector<unsigned short>& wh, const std::vector<float>& t, int widthP) {
        out.off_wh[l] = out.planes.size();
        out.planes.insert(out.planes.end(), wh.begin(), wh.end());
        out.off_tbp[l] = out.tbs.size();
        out.tbs.resize(out.tbs.size() + widthP, 0.f);
        std::copy(t.begin(), t.end(), out.tbs.begin() + out.off_tbp[l]);
    };
    for (int l = 0; l < 6; ++l) {       // the model's layer order: xyz layers 0..2 (blob blocks 0, 2, 4), semantic 3..5
        const FoldedBlock& k = n.blk[l < 3 ? 2 * l : 2 * (l - 3) + 1];
        const int cin = k.cols, cout = k.cout, coutP = p32(cout);
        out.cinP[l] = p32(cin);
        out.coutP[l] = coutP;
        auto value = [&k, cin, cout, coutP](int row, int ch) {
            const bool brow = row >= coutP;                         // b rows follow the a rows
            const int oc = brow ? row - coutP : row;
            return oc < cout && ch < cin ? (brow ? k.b : k.a)[(size_t)oc * cin + ch] : 0.f;
        };
        append(l, pack_fragments<2>(2 * coutP / 16, out.cinP[l] / 32, false, value, split2_host), k.t, coutP);
    }
    {   // conv_end on cat(xyz3 [F3P], sem3 [F3P]): input channel F3P + c is the reference's f3 + c
        const FoldedBlock& k = n.blk[6];
        const int f3 = d.filters_3, F3P = p32(f3);
        out.F3P = F3P;
        auto value = [&k, f3, F3P](int oc, int ch) {
            const int half = ch >= F3P ? 1 : 0, c = ch - half * F3P;
            return oc < f3 && c < f3 ? k.a[(size_t)oc * 2 * f3 + half * f3 + c] : 0.f;
        };
        append(6, pack_fragments<2>(F3P / 16, 2 * F3P / 32, false, value, split2_host), k.t, F3P);
    }
    out.plane_bytes = (out.planes.size() * 2 + 255) & ~(size_t)255;
    return out;
}

}  // namespace sgpr

// Pair-coupled tail of SG.forward on gfx950: Neural Tensor Network
// (TenorNetworkModule.forward, reference layers_batch.py:70-83) + fully_connected_first
// / ReLU + scoring_layer / sigmoid (sg_net.py:131-136).
//
//  * score_pairs_kernel      one wave64 per pair (pair-list mode: eval_batch.py:30-36,
//                            SG.forward's per-pair tail).
//  * ntn_prep_kernel + score_all_pairs_kernel
//                            dense R x M rectangle.  The bilinear form AND the column half of the block term are
//                            hoisted per row graph (A'_r = e1^T W + Wb[:, F:], 16x32; u_r = Wb[:, :F] e1 + bias), so a
//                            pair costs 512 + 256 + 16 FMA.  Both dense layers run on v_mfma_f32_16x16x32_f16 with
//                            two-plane f16 operands (x = hi + lo, 22 bits; three cross products per layer), layer 2
//                            chained off the accumulator layout of layer 1; a wave keeps 4 row graphs in registers and
//                            walks 64-column super-blocks; every store instruction writes 4 rows x 256 contiguous bytes.
// The fused epilogues of that tail (top-k, range selection, mining, positives, threshold counts) follow; what the
// counting one shares with the matrix consumers of sgpr_metrics.hip - the counting steps, the slab layout and its fold,
// the K dispatch of the lists - is sgpr_eval.hpp's.
#include <math.h>

#include <string.h>

#include "sgpr_eval.hpp"
#include "sgpr_map.hpp"

namespace sgpr {

constexpr int F = kF3;   // 32 pooled features
constexpr int T = kT;    // 16 tensor neurons
constexpr int BN_ = kB;  // 16 bottleneck neurons

// ------------------------------------------------------------------ per-pair list
// TenorNetworkModule.forward for one pair on one wave64: lanes with equal t = lane & 15 return the same
// relu(e1^T W[:, :, t] e2 + Wb[t, :] . [e1; e2] + bias[t])      (layers_batch.py:77-83)
//   ntn_w [32][32*16] = weight_matrix.view(F3, -1) (col = j*16 + t),  ntn_wb [16][64],  bias [16]
__device__ __forceinline__ float ntn_neuron(const float* __restrict__ ntn_w, const float* __restrict__ ntn_wb,
                                            const float* __restrict__ bias, const float* __restrict__ e1,
                                            const float* __restrict__ e2, int lane) {
    const int t = lane & 15, q = lane >> 4;
    // v[r] = sum_i e1[i] * W[i][col_r],  col_r = lane + 64 r  ->  j = q + 4r, same t for every r
    float v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = 0.f;
    for (int i = 0; i < F; ++i) {
        const float a = e1[i];
        const float* wr = ntn_w + i * (F * T) + lane;
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = fmaf(a, wr[64 * r], v[r]);
    }
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) s = fmaf(v[r], e2[q + 4 * r], s);
    // block term  Wb[t][:] . [e1; e2], 16 of the 64 products per lane group
    for (int m = 0; m < 16; ++m) {
        const int mm = q * 16 + m;
        const float x = mm < F ? e1[mm] : e2[mm - F];
        s = fmaf(ntn_wb[t * 2 * F + mm], x, s);
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    return relu_keep_nan(s + bias[t]);
}

__global__ __launch_bounds__(256) void score_pairs_kernel(const DevWeights w, const float* __restrict__ p1,
                                                          const int32_t* __restrict__ i1,
                                                          const float* __restrict__ p2,
                                                          const int32_t* __restrict__ i2, int64_t P,
                                                          float* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= P) return;
    const int64_t r1 = i1 ? i1[pair] : pair;
    const int64_t r2 = i2 ? i2[pair] : pair;
    const int t = lane & 15;
    const float h = ntn_neuron(w.ntn_w, w.ntn_wb, w.ntn_bias, p1 + r1 * F, p2 + r2 * F, lane);
    // fully_connected_first + ReLU: lane t computes output neuron t
    float gacc = w.fc1_b[t];
    for (int tt = 0; tt < T; ++tt) gacc = fmaf(w.fc1_w[t * T + tt], __shfl(h, tt), gacc);
    float z = relu_keep_nan(gacc) * w.fc2_w[t];
    z += __shfl_xor(z, 1);
    z += __shfl_xor(z, 2);
    z += __shfl_xor(z, 4);
    z += __shfl_xor(z, 8);
    if (lane == 0) score[pair] = 1.f / (1.f + expf(-(z + w.fc2_b[0])));
}

// stand-alone TenorNetworkModule.forward: out [B][16] = the similarity vector before the FC head
__global__ __launch_bounds__(256) void ntn_kernel(const float* __restrict__ ntn_w, const float* __restrict__ ntn_wb,
                                                  const float* __restrict__ bias, const float* __restrict__ e1,
                                                  const float* __restrict__ e2, int64_t B, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= B) return;
    const float h = ntn_neuron(ntn_w, ntn_wb, bias, e1 + pair * F, e2 + pair * F, lane);
    if (lane < T) out[pair * T + lane] = h;
}

int launch_ntn(const float* w, const float* wb, const float* bias, const float* e1, const float* e2, int64_t B,
               float* out, hipStream_t stream) {
    if (B == 0) return SGPR_OK;
    const int64_t blocks = (B + 3) / 4;
    if (blocks > 0x7fffffffLL) {
        set_error("sgpr_ntn: too many pairs for one launch");
        return SGPR_E_INVALID;
    }
    hipLaunchKernelGGL(ntn_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, w, wb, bias, e1, e2, B, out);
    return launched("ntn_kernel launch");
}

int launch_score_pairs(const sgpr_handle* h, const float* p1, const int32_t* i1, const float* p2, const int32_t* i2,
                       int64_t P, float* score, hipStream_t stream) {
    if (P == 0) return SGPR_OK;
    const int64_t blocks = (P + 3) / 4;
    if (blocks > 0x7fffffffLL) {
        set_error("sgpr_score_pairs: too many pairs for one launch");
        return SGPR_E_INVALID;
    }
    hipLaunchKernelGGL(score_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, h->w, p1, i1, p2, i2, P, score);
    return launched("score_pairs_kernel launch");
}

// ------------------------------------------------------------------ dense all-pairs
// workspace layout:  ur [R][T] f32 | rng [NWG][4] f32 | Ab [R][2][64][8] f16 | Cb [NSB][2][4][64][8] f16
//   ur   u_r[t] = Wb[t][:F] . e1_r + bias[t]
//   Ab   A'_r[t][j] = sum_i e1_r[i] W[i][j][t] + Wb[t][F + j]  as two f16 planes (hi = RNE(a), lo = RNE(a - hi): 22 bits)
//        in MFMA A-operand order: lane (g = j >> 3, l15 = t) holds j = 8g .. 8g+7 -> a wave's operand = 1 KB contiguous
//   Cb   column vectors e2_c as two f16 planes in MFMA B-operand order, 64 columns per super-block: block b (0..3) of a
//        super-block feeds MFMA column l15 with graph column 64 sb + 4 l15 + b, so that after the head a lane owns four
//        CONSECUTIVE columns of one row (one 16-byte store); lane (g, l15) holds j = 8g .. 8g+7
//   rng  per prep workgroup: max |A'|, max |u|, max |e2| - the main kernel derives a bound on every f16 it will form
// f16 has 11 significant bits and a 65504 range: inputs whose bound reaches that range take the exact fp32 per-pair
// path inside score_all_pairs_kernel (never on real data: |pooled| ~ 10); subnormal lo planes are honoured by the
// matrix core (tools/probes/f16_split_probe.hip), so small values only lose what fp32 would lose as well.
constexpr int AP_RW = 4;       // row graphs per wave: their A' operands (2 planes) stay in registers
constexpr int AP_ROWS = 16;    // row graphs per workgroup: 4 waves x AP_RW
constexpr int AP_SB = 64;      // columns per super-block (4 MFMA column blocks)
constexpr int AP_COLS = 256;   // column graphs per work item (4 super-blocks)
#ifndef SGPR_AP_OCC
#define SGPR_AP_OCC 4
#endif
// the multi-rectangle kernel carries the job table on top: at four workgroups per CU (128 VGPRs) it spills 360 bytes per
// lane, at three (166 VGPRs) nothing - config 4's tail 368.5 -> 358.9 us on one box (profiles/r05_tail_variants.txt)
constexpr int AP_MULTI_OCC = 3;
constexpr int AP_OCC = SGPR_AP_OCC;   // resident workgroups per CU the kernel is compiled for (waves per SIMD)
#ifndef SGPR_AP_NI
#define SGPR_AP_NI 2            // (same-box A/B, round 5: 97.7 -> 96.5 us per KITTI-00 matrix, twice; bit-identical - program order only)
#endif
#ifndef SGPR_AP_CHAINS
#define SGPR_AP_CHAINS 1        // 2: layer 1's correction products (lo.hi, hi.lo) in an accumulator chain of their own, met by the
#endif                          // hi.hi chain in one vector add - a shorter dependent chain for four more vector instructions per
                                // (row, block); A/B builds (tools/build_variant.sh): measured slower, profiles/r05_tail_variants.txt
#ifndef SGPR_AP_NT_STORE
#define SGPR_AP_NT_STORE 0      // 1: the matrix leaves through non-temporal stores (A/B builds, tools/build_variant.sh)
#endif
constexpr int AP_NI = SGPR_AP_NI;   // row graphs interleaved in program order (see score_all_pairs_kernel)
constexpr float AP_F16_SAFE = 60000.f;

static inline int ap_prep_groups(int R, int M) {
    const int msb = (M + AP_SB - 1) / AP_SB * AP_SB;
    return ((R > msb ? R : msb) + 15) / 16;
}

// (sized for the three bf16 planes of the wide-range instance, score_all_pairs_wide_kernel; the default two f16 planes
//  use two thirds of the operand regions)
size_t score_all_pairs_ws_bytes(int R, int M) {
    const size_t nsb = (size_t)(M + AP_SB - 1) / AP_SB;
    return (size_t)R * T * sizeof(float) + (size_t)2 * ap_prep_groups(R, M) * 4 * sizeof(float) +
           (size_t)R * 3 * 64 * 8 * sizeof(unsigned short) + nsb * 3 * 4 * 64 * 8 * sizeof(unsigned short);
}

// the operand regions of that layout in a workspace: R rows of `planes` planes (2, or 3 for the wide-range instance) and
// nrng prep groups (a rectangle's 2 ap_prep_groups; the pair list carves its own count and takes Cb as its Cg)
struct ApOperands {
    float* ur;
    float* rng;
    unsigned short* Ab;
    unsigned short* Cb;
};
static ApOperands ap_operands(void* ws, int R, int nrng, int planes) {
    ApOperands o;
    o.ur = static_cast<float*>(ws);
    o.rng = o.ur + (size_t)R * T;
    o.Ab = reinterpret_cast<unsigned short*>(o.rng + (size_t)nrng * 4);
    o.Cb = o.Ab + (size_t)R * planes * 64 * 8;
    return o;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void split2_f16(float a, _Float16& h, _Float16& l) {
    h = (_Float16)a;                       // round to nearest even
    l = (_Float16)(a - (float)h);          // exact residual, rounded once: |a - (h + l)| <= 2^-23 |a| (or 2^-25 absolute)
}

// x = hi + mid + lo EXACTLY, as three bf16 planes: each plane is the upper half of what is left (truncation: 8 + 8 + 8 bits =
// fp32's 24 significant bits; every plane carries x's sign, so a ReLU of x is a ReLU of each plane)
__device__ __forceinline__ void split3_bf16(float x, unsigned& hb, unsigned& mb, unsigned& lb) {
    hb = __float_as_uint(x);
    const float r1 = x - __uint_as_float(hb & 0xffff0000u);
    mb = __float_as_uint(r1);
    const float r2 = r1 - __uint_as_float(mb & 0xffff0000u);
    lb = __float_as_uint(r2);                // (the plane is the upper 16 bits of each word)
}

// max(m, |x|) of the range partials, with +infinity standing for a NaN x: fmaxf drops a NaN, and infinity fails every bound
// of ap_mode, so a launch that met one takes the exact fp32 path (whose ReLU keeps it: relu_keep_nan)
__device__ __forceinline__ float range_max(float m, float x) { return fmaxf(m, x != x ? INFINITY : fabsf(x)); }

__device__ __forceinline__ float wave_max_f32(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    v = fmaxf(v, __shfl_xor(v, 2));
    v = fmaxf(v, __shfl_xor(v, 4));
    v = fmaxf(v, __shfl_xor(v, 8));
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}

// 16 graphs per pair of workgroups.  Row graphs get A' (16 x 32 per graph) as ONE small GEMM per workgroup,
// [16 graphs x 32] x [32 x 512] on the fp32 matrix cores - the 64 KB weight tensor crosses L2 -> CU once per 16 graphs
// instead of once per graph - plus the column half of the block term, split into two f16 planes on the way out, and
// u_r; column graphs get their two-plane copy in super-block order (columns past M are zero-filled).
// LIST (pair-list mode, score_pair_list_kernel): the R row graphs are rows[row_ids[0 .. R)] (the distinct row graphs of
// the list, gathered) and the column operands are laid out per graph, Cb [M][2 planes][32] f16, instead of per super-block.
// NPL: operand planes - 2 (f16: x = hi + lo, 22 bits) or 3 (bf16, the wide-range instance: x exactly, fp32's range)
template <bool LIST, int NPL = 2>
__device__ __forceinline__ void ntn_prep_body(const DevWeights& w, const float* __restrict__ rows, int R,
                                              const float* __restrict__ cols, int M, unsigned short* __restrict__ Ab,
                                              float* __restrict__ ur, float* __restrict__ rng,
                                              unsigned short* __restrict__ Cb, const int block,
                                              const int32_t* __restrict__ row_ids = nullptr) {
    __shared__ float red[4][4];
    __shared__ __attribute__((aligned(16))) unsigned short stage[16 * NPL * 4 * 8 * 8];   // [graph][plane][j >> 3][t & 7][j & 7]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    // two workgroups per 16 graphs (half of the 32 output tiles each): twice the resident waves for a latency-bound job
    const int g0 = (block >> 1) * 16, half = block & 1;
    float amax = 0.f, umax = 0.f, emax = 0.f, l1max = 0.f;       // l1max: max over (graph, t) of sum_j |A'[t][j]|
    if (g0 < R) {
        // A operand: E[g0 + l15][16 blk + 4 lq .. +3] (k order permuted: lane group q supplies k = 4q + s at step s)
        const int ga = min(g0 + l15, R - 1);
        const float* e = rows + (size_t)(LIST ? row_ids[ga] : ga) * F + 4 * lq;
        const float4 ea0 = *reinterpret_cast<const float4*>(e), ea1 = *reinterpret_cast<const float4*>(e + 16);
        // the wave's four output tiles: all 32 weight operands (and the four block-term values) are requested before the
        // first matrix instruction - one L2 round trip for the workgroup's critical path instead of four
        float wv[4][8], wbv[4], l1r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int tile = half * 16 + wave * 4 + q;
            const int t = tile >> 1, j = (tile & 1) * 16 + l15;
            const float* wp = w.ntn_wt + ((size_t)(4 * lq) * T + t) * F + j;            // Wt[i = 4 lq + s][t][j]
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                wv[q][s4] = wp[s4 * T * F];
                wv[q][4 + s4] = wp[(16 + s4) * T * F];
            }
            wbv[q] = w.ntn_wb[t * 2 * F + F + j];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int tile = half * 16 + wave * 4 + q;
            const int t = tile >> 1, j = (tile & 1) * 16 + l15;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea0.x, wv[q][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea0.y, wv[q][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea0.z, wv[q][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea0.w, wv[q][3], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea1.x, wv[q][4], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea1.y, wv[q][5], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea1.z, wv[q][6], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea1.w, wv[q][7], acc, 0, 0, 0);
            // acc[r] = (e1^T W)_{g0 + 4 lq + r}[t][j]; the column half of the block term rides along: A' = A + Wb[t][F + j]
            const float wbc = wbv[q];
            // tiles q = 0, 1 (and 2, 3) are the two halves j < 16 / j >= 16 of the same t: a row of A' is the 16 lanes of
            // a lane group in both of them
            if ((q & 1) == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) l1r[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int g = g0 + 4 * lq + r;
                if (g < R) {
                    const float a = acc[r] + wbc;
                    amax = range_max(amax, a);
                    l1r[r] += fabsf(a);
                    // staged through LDS in the operand layout: the lanes hold one f16 each of a 16-byte operand unit
                    // (8 consecutive j of one (graph, plane, t)); 2-byte global stores cost the kernel a quarter of its time
                    unsigned short* dst = stage + (((4 * lq + r) * NPL * 4 + (j >> 3)) * 8 + (t & 7)) * 8 + (j & 7);
                    if constexpr (NPL == 3) {
                        unsigned hb, mb, lb;
                        split3_bf16(a, hb, mb, lb);
                        dst[0] = (unsigned short)(hb >> 16);
                        dst[4 * 8 * 8] = (unsigned short)(mb >> 16);
                        dst[2 * 4 * 8 * 8] = (unsigned short)(lb >> 16);
                    } else {
                        _Float16 h, l;
                        split2_f16(a, h, l);
                        dst[0] = __builtin_bit_cast(unsigned short, h);
                        dst[4 * 8 * 8] = __builtin_bit_cast(unsigned short, l);
                    }
                }
            }
            if (q & 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = l1r[r];
                    v += __shfl_xor(v, 1);
                    v += __shfl_xor(v, 2);
                    v += __shfl_xor(v, 4);
                    v += __shfl_xor(v, 8);
                    l1max = fmaxf(l1max, v);
                }
            }
        }
    }
    if (g0 < R) {
        __syncthreads();
        // 16 graphs x 2 planes x 4 (j >> 3) x 8 t of this half = 1024 units of 16 bytes, 8 consecutive t contiguous in memory
        for (int u = threadIdx.x; u < 16 * NPL * 4 * 8; u += 256) {
            const int tl = u & 7, jb = (u >> 3) & 3, pl = (u >> 5) % NPL, gi = (u >> 5) / NPL;
            if (g0 + gi < R)
                *reinterpret_cast<uint4*>(Ab + (((size_t)(g0 + gi) * NPL + pl) * 64 + jb * 16 + half * 8 + tl) * 8) =
                    *reinterpret_cast<const uint4*>(stage + (size_t)u * 8);
        }
    }
    // block term of the row graphs and the column operands: one graph per wave pass
    for (int gi = half * 8 + wave * 2; gi < half * 8 + wave * 2 + 2; ++gi) {
        const int g = g0 + gi;
        if (g < R) {
            const float* e1 = rows + (size_t)(LIST ? row_ids[g] : g) * F;
            float s = 0.f;
            for (int m = 0; m < 8; ++m) s = fmaf(w.ntn_wb[l15 * 2 * F + lq * 8 + m], e1[lq * 8 + m], s);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            s += w.ntn_bias[l15];
            umax = range_max(umax, s);
            if (lq == 0) ur[(size_t)g * T + l15] = s;
        }
        const int msb = LIST ? M : (M + AP_SB - 1) / AP_SB * AP_SB;
        if (g < msb && lane < F) {                          // the column operand itself, two f16 planes (zeros past M)
            const float x = g < M ? cols[(size_t)g * F + lane] : 0.f;
            emax = range_max(emax, x);
            _Float16 h, l;
            split2_f16(x, h, l);
            if (LIST) {
                unsigned short* dst = Cb + (size_t)g * (2 * F) + lane;
                dst[0] = __builtin_bit_cast(unsigned short, h);
                dst[F] = __builtin_bit_cast(unsigned short, l);
            } else {
                const int sb = g >> 6, cl = g & 63, c15 = cl >> 2, b = cl & 3, j = lane;
                unsigned short* dst = Cb + ((((size_t)sb * NPL) * 4 + b) * 64 + (j >> 3) * 16 + c15) * 8 + (j & 7);
                if constexpr (NPL == 3) {
                    unsigned hb, mb, lb;
                    split3_bf16(x, hb, mb, lb);
                    dst[0] = (unsigned short)(hb >> 16);
                    dst[4 * 64 * 8] = (unsigned short)(mb >> 16);
                    dst[2 * 4 * 64 * 8] = (unsigned short)(lb >> 16);
                } else {
                    dst[0] = __builtin_bit_cast(unsigned short, h);
                    dst[4 * 64 * 8] = __builtin_bit_cast(unsigned short, l);
                }
            }
        }
    }
    // (a NaN among A', u or e2 sits in its maximum as +infinity, range_max; l1max needs none of its own: a row of A' with a
    //  NaN has marked amax)
    amax = wave_max_f32(amax);
    umax = wave_max_f32(umax);
    emax = wave_max_f32(emax);
    l1max = wave_max_f32(l1max);
    if (lane == 0) {
        red[wave][0] = amax;
        red[wave][1] = umax;
        red[wave][2] = emax;
        red[wave][3] = l1max;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        rng[(size_t)block * 4 + q] = fmaxf(fmaxf(red[0][q], red[1][q]), fmaxf(red[2][q], red[3][q]));
    }
}

__global__ __launch_bounds__(256) void ntn_prep_kernel(const DevWeights w, const float* __restrict__ rows, int R,
                                                       const float* __restrict__ cols, int M,
                                                       unsigned short* __restrict__ Ab, float* __restrict__ ur,
                                                       float* __restrict__ rng, unsigned short* __restrict__ Cb) {
    ntn_prep_body<false>(w, rows, R, cols, M, Ab, ur, rng, Cb, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void ntn_prep_wide_kernel(const DevWeights w, const float* __restrict__ rows, int R,
                                                            const float* __restrict__ cols, int M,
                                                            unsigned short* __restrict__ Ab, float* __restrict__ ur,
                                                            float* __restrict__ rng, unsigned short* __restrict__ Cb) {
    ntn_prep_body<false, 3>(w, rows, R, cols, M, Ab, ur, rng, Cb, (int)blockIdx.x);
}

// several independent rectangles in one launch (sgpr_score_all_pairs_multi): job j owns the prep workgroups
// [block0[j], block0[j+1]) and the work items [item0[j], item0[j+1]) of the main kernel
constexpr int AP_MAX_JOBS = 8;
struct ApJob {
    const float* rows;
    const float* cols;
    float* score;
    int64_t ld;
    unsigned short* Ab;
    unsigned short* Cb;
    float* ur;
    float* rng;
    int R, M, nrng;
};
struct ApJobs {
    int n;
    int block0[AP_MAX_JOBS + 1];
    int item0[AP_MAX_JOBS + 1];
    ApJob job[AP_MAX_JOBS];
};

__global__ __launch_bounds__(256) void ntn_prep_multi_kernel(const DevWeights w, const ApJobs jobs) {
    int j = 0;
    while (j + 1 < jobs.n && (int)blockIdx.x >= jobs.block0[j + 1]) ++j;
    const ApJob& q = jobs.job[j];
    ntn_prep_body<false>(w, q.rows, q.R, q.cols, q.M, q.Ab, q.ur, q.rng, q.Cb, (int)blockIdx.x - jobs.block0[j]);
}

__device__ __forceinline__ f32x4 mfma_f16(f16x8 a, f16x8 b, f32x4 c) {
    // 16x16x32: D[4*(l>>4)+r][l&15] += sum_k A[row][k] B[k][col]; lane l supplies A[l&15][8*(l>>4) .. +7] and
    // B[8*(l>>4) .. +7][l&15]
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// v_permlane32_swap: lanes 32-63 of the first operand trade places with lanes 0-31 of the second; the sum of the two
// results is, in the lower half, a[l] + a[l+32] and, in the upper half, b[l-32] + b[l]
__device__ __forceinline__ float swap32_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// v_permlane16_swap: odd 16-lane rows of the first operand trade places with even rows of the second; the sum is
// a[l] + a[l+16] in even rows and b[l-16] + b[l] in odd rows
__device__ __forceinline__ float swap16_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ReLU as ONE instruction: fmaxf (and fmed3 with an infinite bound, which the optimizer folds back into it) first
// canonicalises the operand with a second v_max x, x.  A signed-integer max with 0 does the same job on the bit
// pattern: every negative float (and -0) is a negative integer.
__device__ __forceinline__ float relu(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

// relu(h[0..3]) -> the layer-2 B operand {hi01, hi23, lo01, lo23} (packed f16 planes, hi + lo = relu(h) to 22 bits):
//   hi = the values truncated to f16 (v_cvt_pkrtz_f16_f32: |hi| <= |h|, same sign)
//   lo = f16(h - hi) straight out of one mixed-precision FMA per value (v_fma_mixlo/mixhi_f16: f16 * f32 + f32, the f16
//        result written to one half of the destination)
//   truncation makes both planes carry h's sign, so the ReLU is one packed SIGNED-INTEGER max with 0 per plane pair
//   (v_pk_max_i16: a negative f16 is a negative int16; no canonicalising pre-pass like the float max gets).
// Only the four mix instructions are inline asm (the compiler has no builtin for them): the conversions before and the
// maxima after are visible instructions, so the wait states an MFMA result needs before a vector read and a vector
// result needs before an MFMA read are inserted by the compiler - it does not look inside inline asm (a first version
// with everything in asm read half-written accumulators).
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// CL: the low plane's ReLU as the `clamp` bit of the instruction that forms it.  lo = h - hi lies in [0, ulp(hi)) for
// h >= 0 and in (-ulp(hi), 0] for h < 0 (hi truncates towards zero), and clamp cuts to [0, 1]: exact whenever ulp(hi) <= 1,
// i.e. |h| < 2048 - which the launch guarantees through a bound on |H| (ap_mode) before it picks this variant.
template <bool CL>
__device__ __forceinline__ f16x8 split_relu4(f32x4 h) {
    const unsigned h01 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(h[0], h[1]));
    const unsigned h23 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(h[2], h[3]));
    unsigned l01, l23;
    const i16x2 z = {0, 0};
    const unsigned a = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, h01), z));
    const unsigned b = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, h23), z));
    if constexpr (CL) {
        asm("v_fma_mixlo_f16 %0, %2, -1.0, %4 op_sel_hi:[1,0,0] clamp\n\t"
            "v_fma_mixlo_f16 %1, %3, -1.0, %6 op_sel_hi:[1,0,0] clamp\n\t"
            "v_fma_mixhi_f16 %0, %2, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0] clamp\n\t"
            "v_fma_mixhi_f16 %1, %3, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0] clamp"
            : "=&v"(l01), "=&v"(l23)
            : "v"(h01), "v"(h23), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]));
        return __builtin_bit_cast(f16x8, u32x4{a, b, l01, l23});
    } else {
        asm("v_fma_mixlo_f16 %0, %2, -1.0, %4 op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixlo_f16 %1, %3, -1.0, %6 op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %0, %2, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %1, %3, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
            : "=&v"(l01), "=&v"(l23)
            : "v"(h01), "v"(h23), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]));
        const unsigned c = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, l01), z));
        const unsigned d = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, l23), z));
        return __builtin_bit_cast(f16x8, u32x4{a, b, c, d});
    }
}

// Exact fp32 evaluation of the rectangle [r0, r1) x [c0, c1), one pair per wave iteration, for inputs outside the f16
// range.  Deliberately rolled loops: it shares the kernel with the hot loop and must not cost it registers.
__device__ __forceinline__ float slow_pair(const DevWeights& w, const float* __restrict__ e1, const float* __restrict__ e2) {
    const int lane = threadIdx.x & 63, t = lane & 15, q = lane >> 4;
    float s = 0.f;
#pragma unroll 1
    for (int j = 8 * q; j < 8 * q + 8; ++j) {                     // this lane group's quarter of the 32 j
        float v = 0.f;
#pragma unroll 1
        for (int i = 0; i < F; ++i) v = fmaf(e1[i], w.ntn_w[i * (F * T) + j * T + t], v);
        s = fmaf(v, e2[j], s);
    }
#pragma unroll 1
    for (int m = 16 * q; m < 16 * q + 16; ++m) s = fmaf(w.ntn_wb[t * 2 * F + m], m < F ? e1[m] : e2[m - F], s);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    const float h = relu_keep_nan(s + w.ntn_bias[t]);
    float gacc = w.fc1_b[t];
#pragma unroll 1
    for (int tt = 0; tt < T; ++tt) gacc = fmaf(w.fc1_w[t * T + tt], __shfl(h, tt), gacc);
    float z = relu_keep_nan(gacc) * w.fc2_w[t];
    z += __shfl_xor(z, 1);
    z += __shfl_xor(z, 2);
    z += __shfl_xor(z, 4);
    z += __shfl_xor(z, 8);
    return 1.f / (1.f + expf(-(z + w.fc2_b[0])));
}

__device__ __forceinline__ void slow_tile(const DevWeights& w, const float* __restrict__ prow,
                                          const float* __restrict__ pcol, int r0, int r1, int c0, int c1,
                                          float* __restrict__ score, int64_t ld) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = r0; r < r1; ++r)
#pragma unroll 1
        for (int c = c0; c < c1; ++c) {
            const float sc = slow_pair(w, prow + (size_t)r * F, pcol + (size_t)c * F);
            if (lane == 0) score[(size_t)r * ld + c] = sc;
        }
}

// One wave owns AP_RW = 4 row graphs - their A' operands (two f16 planes) are fetched once per work item and kept in
// registers - and walks super-blocks of 64 column graphs, whose operands (0.6 MB in total: L2-resident) are fetched
// one 16-column block ahead.  Per (row, block of 16 columns):
//   layer 1  H[t][c] = relu(u_r[t] + sum_j A'_r[t][j] e2_c[j]),  K = 32: three f16 MFMAs (lo.hi, hi.lo, hi.hi) on the
//            accumulator initialised with u_r - no vector instruction at all
//   layer 2  G[o][c] = relu(b1[o] + sum_t W1[o][t] H[t][c])   two f16 MFMAs: H is consumed straight from the
//            accumulator layout (lane group g holds t = 4g..4g+3), split into two f16 planes; the K slots
//            8g..8g+3 / 8g+4..8g+7 carry hi / lo, the A operand is W1 laid out to match
//   head     z[c] = b2 + sum_o w2[o] G[o][c]: w2 is folded into layer 2 (ap_consts), so a lane's four terms are four
//            v_med3_f32 of the accumulator against its own side of zero and three adds; then per super-block a lane-swap
//            transpose-reduce over the 4 lane groups leaves lane (g, l15) with row g, columns 4 l15 .. 4 l15 + 3:
//            sigmoid, one 16-byte store.
// OCC = resident workgroups per CU the instance is compiled for; NI = row graphs whose dependent MFMA -> vector ->
// MFMA -> vector chains are interleaved in program order (1, 2 or 4); VAR = timing experiments only (tools/probes):
// bit 1 drops the stores, bit 2 the operand loads of the next block, bit 4 (16) the matrix instructions, bit 5 (32) the
// vector work between them
// per-wave constants of the tail: the head's weights in the lane layout of the MFMA results
struct ApConsts {
    f16x8 w1hi, w1lo;
    float4 b1v, side;
    float nb2, nl2e;
};

// The head's weight w2[o] is folded into layer 2 (row o of W1 and b1[o] scaled by it - in fp32, before the planes are
// cut), so that the accumulator holds q''[o] = w2[o] (b1[o] + W1[o].H) and the pair's term w2[o] relu(q[o]) is q''[o]
// clamped to its own side of zero: max(q'', 0) for w2 > 0, min(q'', 0) for w2 < 0 = ONE v_med3_f32 against
// (0, side[o]), side = +inf / -inf - instead of an integer maximum and a multiply-add per value.
// Both are also scaled by the handle's power of two head_scale (head_range, sgpr_internal.hpp: the largest fold weight
// in [2^14, 2^15), so that no low plane is an f16 subnormal), undone exactly in the sigmoid's constant nl2e.
__device__ __forceinline__ ApConsts ap_consts(const DevWeights& w, int l15, int g) {
    ApConsts c;
    const float s = w.fc2_w[l15] * w.head_scale;                                       // the A operand's row is o = l15
    float4 w1v = *reinterpret_cast<const float4*>(w.fc1_w + l15 * T + 4 * g);         // W1[o = l15][t = 4g..4g+3]
    w1v = make_float4(s * w1v.x, s * w1v.y, s * w1v.z, s * w1v.w);
    const _Float16 wh0 = (_Float16)w1v.x, wh1 = (_Float16)w1v.y, wh2 = (_Float16)w1v.z, wh3 = (_Float16)w1v.w;
    const _Float16 z16 = (_Float16)0.f;
    c.w1hi = f16x8{wh0, wh1, wh2, wh3, wh0, wh1, wh2, wh3};                      // meets H's hi and lo planes
    c.w1lo = f16x8{(_Float16)(w1v.x - (float)wh0), (_Float16)(w1v.y - (float)wh1), (_Float16)(w1v.z - (float)wh2),
                        (_Float16)(w1v.w - (float)wh3), z16, z16, z16, z16};            // meets the hi plane only
    const float4 b1 = *reinterpret_cast<const float4*>(w.fc1_b + 4 * g);              // the accumulator's rows are o = 4g + r
    const float4 w2 = *reinterpret_cast<const float4*>(w.fc2_w + 4 * g);
    const float hs = w.head_scale;
    c.b1v = make_float4((w2.x * hs) * b1.x, (w2.y * hs) * b1.y, (w2.z * hs) * b1.z, (w2.w * hs) * b1.w);
    c.side = make_float4(w2.x < 0.f ? -INFINITY : INFINITY, w2.y < 0.f ? -INFINITY : INFINITY,
                         w2.z < 0.f ? -INFINITY : INFINITY, w2.w < 0.f ? -INFINITY : INFINITY);
    c.nb2 = -w.fc2_b[0] * 1.4426950408889634f;
    c.nl2e = w.head_nl2e;                                 // -log2(e) / head_scale: fmaf(2^k z, nl2e, nb2) = fmaf(z, -log2 e, nb2)
    return c;
}

// max |A'|, max |u|, max |e2| partials -> can every f16 the launch forms be represented?
// The whole workgroup reads the partials, four independent 16-byte loads per thread and round (a wave reading them alone,
// one dependent load per loop trip, spent ~0.7 us per 64 partials before its first matrix instruction: 6 us of the
// KITTI-00 tail, 25 us of a 12 k-graph pair list); the waves' maxima meet in LDS.  Every wave returns the same values.
__device__ __forceinline__ void ap_range(const float* __restrict__ rng, int nrng, float& am, float& um, float& em, float& l1) {
    __shared__ float4 part[4];
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < nrng; i += 4 * 256) {
        const float4 v0 = *reinterpret_cast<const float4*>(rng + (size_t)i * 4);
        const float4 v1 = i + 256 < nrng ? *reinterpret_cast<const float4*>(rng + (size_t)(i + 256) * 4) : z;
        const float4 v2 = i + 512 < nrng ? *reinterpret_cast<const float4*>(rng + (size_t)(i + 512) * 4) : z;
        const float4 v3 = i + 768 < nrng ? *reinterpret_cast<const float4*>(rng + (size_t)(i + 768) * 4) : z;
        am = fmaxf(fmaxf(am, v0.x), fmaxf(fmaxf(v1.x, v2.x), v3.x));
        um = fmaxf(fmaxf(um, v0.y), fmaxf(fmaxf(v1.y, v2.y), v3.y));
        em = fmaxf(fmaxf(em, v0.z), fmaxf(fmaxf(v1.z, v2.z), v3.z));
        l1 = fmaxf(fmaxf(l1, v0.w), fmaxf(fmaxf(v1.w, v2.w), v3.w));
    }
    am = wave_max_f32(am);
    um = wave_max_f32(um);
    em = wave_max_f32(em);
    l1 = wave_max_f32(l1);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = make_float4(am, um, em, l1);
    __syncthreads();
    const float4 p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3];
    am = fmaxf(fmaxf(p0.x, p1.x), fmaxf(p2.x, p3.x));
    um = fmaxf(fmaxf(p0.y, p1.y), fmaxf(p2.y, p3.y));
    em = fmaxf(fmaxf(p0.z, p1.z), fmaxf(p2.z, p3.z));
    l1 = fmaxf(fmaxf(p0.w, p1.w), fmaxf(p2.w, p3.w));
    __syncthreads();                                      // (the multi-job kernel calls this once per rectangle)
}
// 0: exact fp32 per-pair path (an f16 of the launch could overflow); 1: the f16-plane path; 2: the same with the low
// plane's ReLU folded into its conversion (split_relu4<true>): |H[t]| <= |u[t]| + sum_j |A'[t][j]| max|e2| < 1024
__device__ __forceinline__ int ap_mode(float am, float um, float em, float l1) {
    if (!((am < AP_F16_SAFE) && (em < AP_F16_SAFE) && (um + 32.f * am * em < AP_F16_SAFE))) return 0;
    return (um + l1 * em < 1024.f) ? 2 : 1;
}

// ------------------------------------------------------------------ fused top-k epilogue (sgpr_score_topk)
// Instead of storing a super-block's scores, the instance with TK > 0 feeds them to a per-row top-TK list:
//   TK = 1   every lane keeps the best (score, column) of ITS columns of row g in two registers (columns reach a lane in
//            ascending order, so a strict comparison keeps the lower column of a tie); the 16 lanes of the row meet when
//            the row group is flushed (four xor-shuffles).
//   TK > 1   lane l15 of lane group g holds entry l15 of row g's list (TK <= 16 lanes), the TK-th entry is the row's
//            threshold (two registers).  A column block whose candidates all fail their threshold costs a compare and a
//            ballot; otherwise the 16 candidates of each row and its list are merged by rank (each value counts what beats
//            it - 16 + TK shuffles -) and scattered through 512 bytes of LDS per wave.  No runtime-indexed array: nothing
//            of the list can go to scratch.
// Order: score descending, then column ascending; NaN never qualifies; (-inf, INT_MAX) is an empty slot (written as -1).
// A workgroup's work items are one contiguous row-major range, so it sees every column chunk of the row groups inside
// its range and writes their lists straight to the result; the row groups at its two ends are shared with neighbours and
// go to partial list slots [wg][2][16 rows][k] that topk_merge_kernel folds together: at most R + 32 grid lists.
struct TopkArgs {
    const int32_t* row_self;   // [R] the column index of each query row's own frame, or nullptr: row0 + r
    int row0, window, causal, k, wg;
    float* val;                // [R][k]
    int32_t* idx;
    float* pval;               // [grid][2][AP_ROWS][k] partial lists of the row groups at the ends of a workgroup's range
    int32_t* pidx;
    int32_t* status;           // bit 16: a row_self entry outside [0, M)
};

constexpr int TK_EMPTY = 0x7fffffff;

__device__ __forceinline__ bool tk_beats(float av, int ac, float bv, int bc) { return av > bv || (av == bv && ac < bc); }

// (tk_bounds, the eligibility rule of every list and range epilogue: sgpr_internal.hpp)

// merge the candidate (cv, cc) of every lane (ok: it qualifies) into its lane group's list (entry l15 in (lv, lc));
// sv / sc: this wave's 64-entry LDS slice
template <int K>
__device__ __forceinline__ void tk_merge(float& lv, int& lc, float cv, int cc, bool ok, float* sv, int* sc) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, base = lane & 48;
    if (!ok) {
        cv = -INFINITY;
        cc = TK_EMPTY;
    }
    int rc = 0, rl = l15;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float ov = __shfl(cv, base + j);
        const int oc = __shfl(cc, base + j);
        rc += tk_beats(ov, oc, cv, cc) ? 1 : 0;
        rl += tk_beats(ov, oc, lv, lc) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float ov = __shfl(lv, base + j);
        const int oc = __shfl(lc, base + j);
        rc += tk_beats(ov, oc, cv, cc) ? 1 : 0;
    }
    if (ok && rc < K) {
        sv[base + rc] = cv;
        sc[base + rc] = cc;
    }
    if (l15 < K && rl < K) {
        sv[base + rl] = lv;
        sc[base + rl] = lc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (l15 < K) {
        lv = sv[lane];
        lc = sc[lane];
    }
    __builtin_amdgcn_wave_barrier();
}

// one super-block's scores of row g (lane: columns c0 .. c0 + 3) into the row's list
template <int K>
__device__ __forceinline__ void tk_push(const float (&sc)[4], int c0, int M, int ea, int eb, bool live, float& tv, int& tc,
                                        float& thv, int& thc, float* lsv, int* lsc) {
    if constexpr (K == 1) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = c0 + b;
            const float v = sc[b];
            if (live && c < M && (c < ea || c > eb) && v == v && tk_beats(v, c, tv, tc)) {
                tv = v;
                tc = c;
            }
        }
    } else {
        // (a rolled loop with one merge body spills more, 300 against 248-312 bytes per lane: kept unrolled)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = c0 + b;
            const float v = sc[b];
            const bool q = live && c < M && (c < ea || c > eb) && v == v && tk_beats(v, c, thv, thc);
            if (__any(q)) {
                tk_merge<K>(tv, tc, v, c, q, lsv, lsc);
                const int src = (threadIdx.x & 48) + K - 1;
                thv = __shfl(tv, src);
                thc = __shfl(tc, src);
            }
        }
    }
}

// the lists of row group rg (lane group g of this wave: row r) leave: to the result when this workgroup saw every column
// chunk of the row group, else to partial slot 0 (the row group its range starts in) or 1 (the one it ends in)
// (NEG: the lists hold negated scores - sgpr_score_mine's positives -; the result gets them back, bit for bit)
template <int K, bool NEG = false>
__device__ __forceinline__ void tk_flush(const TopkArgs& a, int rg, int ncc, int it0, int it1, int r, int R, float tv, int tc) {
    const int lane = threadIdx.x & 63, l15 = lane & 15;
    if constexpr (K == 1) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const float ov = __shfl_xor(tv, m);
            const int oc = __shfl_xor(tc, m);
            if (tk_beats(ov, oc, tv, tc)) {
                tv = ov;
                tc = oc;
            }
        }
    }
    if (r >= R || l15 >= a.k) return;
    if ((int64_t)rg * ncc >= it0 && (int64_t)(rg + 1) * ncc <= it1) {
        a.val[(size_t)r * a.k + l15] = NEG ? -tv : tv;
        a.idx[(size_t)r * a.k + l15] = tc == TK_EMPTY ? -1 : tc;
    } else {
        const int slot = rg == it0 / ncc ? 0 : 1;
        const size_t p = ((size_t)(a.wg * 2 + slot) * AP_ROWS + (r - rg * AP_ROWS)) * a.k + l15;
        a.pval[p] = tv;
        a.pidx[p] = tc;
    }
}

// ------------------------------------------------------------------ fused range epilogue (sgpr_score_above)
// Every eligible pair with score >= thr, in row-major order, from two runs of the same kernel instance (TK = TK_ABOVE):
//   pass 1  each lane counts the hits among its four columns of row g; the 16 lanes of the row meet at the flush (four
//           xor-shuffles) and the row's count goes to cnt[r] - or, for the two row groups at the ends of the workgroup's
//           range, to partial slots [wg][2][16 rows] (tk_flush's split).  A super-block with a hit marks its work item in
//           flag[] (a plain byte store of 1: the waves that share the item store the same value).
//   fold + scan  above_fold_kernel adds the partial counts of each shared row and leaves every share's offset within its
//           row in poff; above_scan_kernel turns the counts into row_ptr (int64) and the total.
//   pass 2  re-scores the flagged work items only (an unflagged item holds no hit for any row of its workgroup, so the
//           running positions stay right).  Hit (r, c) goes to row_ptr[r] + (the share's offset) + the hits of row r
//           before it: a running position per row plus, within a super-block, the row's hits of lower lanes (four ballots,
//           masked to the lane group) and of lower columns of the same lane.  Written only below cap.
// Both passes take the same range decision and the same arithmetic (one instance), so they agree hit for hit; pass 2
// checks that (status bit 32).
constexpr int TK_ABOVE = -1;

struct AboveArgs {
    const int32_t* row_self;   // [R] own frame of each row, or nullptr: row0 + r
    int row0, window, causal, pass, wg;
    int rout0;                 // output row index of row 0 (the row block of a long launch)
    float thr;
    unsigned char* flag;       // [items] 1: the work item holds a hit (pass 1 writes, pass 2 reads)
    int32_t* cnt;              // [R] hits per row
    int32_t* pcnt;             // [grid][2][AP_ROWS] hits of the row groups at the ends of a workgroup's range
    int32_t* poff;             // [grid][2][AP_ROWS] where that share starts within its row (above_fold_kernel)
    const int64_t* row_ptr;    // [R + 1] (pass 2)
    int32_t* rows;             // [cap] outputs (pass 2)
    int32_t* cols;
    float* vals;
    int64_t cap;
    int32_t* status;           // bit 16: a row_self entry outside [0, M); bit 32: pass 2 disagreed with pass 1
};

// one super-block's scores of row g (lane: columns c0 .. c0 + 3): pass 1 counts them into cnt and flags the item, pass 2
// writes them from the row's running position pos
__device__ __forceinline__ void ab_push(const AboveArgs& a, const float (&sc)[4], int c0, int M, int ea, int eb, bool live,
                                        int r, int it, int& cnt, long long& pos) {
    bool h[4];
    int nh = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = c0 + b;
        h[b] = live && c < M && (c < ea || c > eb) && sc[b] >= a.thr;
        nh += h[b] ? 1 : 0;
    }
    if (a.pass == 1) {
        cnt += nh;
        if (__any(nh != 0) && (threadIdx.x & 63) == 0) a.flag[it] = 1;
        return;
    }
    if (!__any(nh != 0)) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long gmask = 0xffffull << (lane & 48), below = gmask & ((1ull << lane) - 1ull);
    int before = 0, total = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long B = __ballot(h[b]);
        before += __popcll(B & below);
        total += __popcll(B & gmask);
    }
    long long p = pos + before;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (h[b]) {
            if (p < a.cap) {
                a.rows[p] = a.rout0 + r;
                a.cols[p] = c0 + b;
                a.vals[p] = sc[b];
            }
            ++p;
        }
    }
    pos += total;
}

// row group rg leaves (lane group g of this wave: row r).  Pass 1: the row's count to cnt[r], or to partial slot 0 / 1
// when the row group is shared with a neighbouring workgroup.  Pass 2: the hits written must equal that count.
__device__ __forceinline__ void ab_flush(const AboveArgs& a, int rg, int ncc, int it0, int it1, int r, int R, int cnt,
                                         long long pos, long long start) {
    const int l15 = threadIdx.x & 15;
    const bool inside = (int64_t)rg * ncc >= it0 && (int64_t)(rg + 1) * ncc <= it1;
    const size_t p = ((size_t)(a.wg * 2 + (rg == it0 / ncc ? 0 : 1))) * AP_ROWS + (r - rg * AP_ROWS);
    if (a.pass == 1) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) cnt += __shfl_xor(cnt, m);
        if (r >= R || l15 != 0) return;
        if (inside) a.cnt[r] = cnt;
        else a.pcnt[p] = cnt;
    } else {
        if (r >= R || l15 != 0) return;
        if (pos - start != (inside ? a.cnt[r] : a.pcnt[p])) atomicOr(a.status, 32);
    }
}

// pass 2: where row r's hits of this workgroup start
__device__ __forceinline__ long long ab_start(const AboveArgs& a, int rg, int ncc, int it0, int it1, int r, int R) {
    if (r >= R) return 0;
    const bool inside = (int64_t)rg * ncc >= it0 && (int64_t)(rg + 1) * ncc <= it1;
    long long s = a.row_ptr[r];
    if (!inside) s += a.poff[((size_t)(a.wg * 2 + (rg == it0 / ncc ? 0 : 1))) * AP_ROWS + (r - rg * AP_ROWS)];
    return s;
}

// ------------------------------------------------------------------ fused evaluation epilogues (sgpr_score_positives,
// sgpr_score_threshold_counts): sgpr_pair_positives / sgpr_pair_threshold_counts on the scores as the tail makes them.
//   TK_POS  every pair is labelled (classify_pair: float64 poses, or the explicit labels); the scores of the positive
//           ones are appended to the output list (one ballot prefix and one global atomic per wave and super-block that
//           holds any), positives with a negative / NaN score are counted instead.
//   TK_CNT  every negative pair is counted between the thresholds and optionally ranked among the positive values with
//           sgpr_eval.hpp's steps - the ones pair_threshold_count_kernel takes on a resident matrix: tree in LDS,
//           wave-aggregated LDS atomics, the workgroup's own slab at the end (no global atomic in the loop), one fold.
// With poses, a work item is first tested as a whole: the bounding box of the wave's four row poses against the box of
// the chunk's 256 column poses (eval_colbox_kernel), float64, the gap cut by 2^-40 of the largest magnitude and the
// squared distance to clear the class boundary by 0.1 % - far beyond the roundings of utils.py:36's arithmetic.  An item
// farther than d_pos from every row holds no positive (TK_POS skips it unscored); one farther than max(d_pos, d_neg)
// holds negatives only (TK_CNT counts it without per-pair float64 arithmetic).  A NaN pose widens its box to the plane.
constexpr int TK_POS = -2;
constexpr int TK_CNT = -3;
constexpr int EV_MAX_T = SGPR_SCORE_COUNT_MAX_THRESHOLDS;   // 2047: tree 8 KB + counters 8 KB + at_least 16 KB of LDS
constexpr int EV_TP = EV_MAX_T + 1;                          // tree nodes (a power of two)

struct EvalArgs {
    PairTruth truth;
    double lo2, hi2, cut_pos, cut_neg;   // squared class boundaries; squared gaps that rule a work item out
    const double* cbox;                  // [ncc][4] column chunk boxes: x lo, x hi, z lo, z hi (pose mode)
    // TK_POS
    float* out;                          // [cap] positive scores, appended
    long long cap;
    unsigned long long* count;           // [0] positives with a usable score, [1] positives with a negative / NaN one
    // TK_CNT
    ThrView th;                          // the thresholds and the workgroup's counters (sgpr_eval.hpp)
    // per lane: labelled pairs skipped for a negative / NaN score, the rank sum
    unsigned nbad;
    unsigned long long rank2;
};

// the pose box of the wave's four rows (lane group g: row r) - wave-uniform after the shuffles
__device__ __forceinline__ void ev_row_box(double px, double pz, double (&bx)[4]) {
    const bool nan = px != px || pz != pz;
    bx[0] = nan ? -INFINITY : px;
    bx[1] = nan ? INFINITY : px;
    bx[2] = nan ? -INFINITY : pz;
    bx[3] = nan ? INFINITY : pz;
#pragma unroll
    for (int m = 16; m < 64; m <<= 1) {
        bx[0] = fmin(bx[0], __shfl_xor(bx[0], m));
        bx[1] = fmax(bx[1], __shfl_xor(bx[1], m));
        bx[2] = fmin(bx[2], __shfl_xor(bx[2], m));
        bx[3] = fmax(bx[3], __shfl_xor(bx[3], m));
    }
}

// squared lower bound of every (row, column) distance of the two boxes, 0 when they may touch (NaN / inf: 0)
__device__ __forceinline__ double ev_gap2(const double (&rb)[4], const double* __restrict__ cb) {
    const double amax = fmax(fmax(fmax(fabs(rb[0]), fabs(rb[1])), fmax(fabs(rb[2]), fabs(rb[3]))),
                             fmax(fmax(fabs(cb[0]), fabs(cb[1])), fmax(fabs(cb[2]), fabs(cb[3]))));
    const double e = amax * 9.094947017729282e-13;          // 2^-40
    const double gx = fmax(fmax(rb[0] - cb[1], cb[0] - rb[1]) - e, 0.0);
    const double gz = fmax(fmax(rb[2] - cb[3], cb[2] - rb[3]) - e, 0.0);
    const double g2 = gx * gx + gz * gz;
    return g2 == g2 ? g2 : 0.0;
}

__device__ __forceinline__ int ev_class(const EvalArgs& e, int r, int c, double px, double pz) {
    return classify_pair(e.truth, r, c, px, pz, e.lo2, e.hi2);
}

// TK_POS: row r's four pairs (r, c0 .. c0 + 3) of one super-block (live: r < R)
__device__ __forceinline__ void ev_pos_push(EvalArgs& e, const float (&sc)[4], int c0, int M, bool live, int r,
                                            double px, double pz) {
    bool p[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = c0 + b;
        p[b] = live && c < M && ev_class(e, r, c, px, pz) == 1;
        if (p[b] && ev_bad(sc[b])) {
            ++e.nbad;
            p[b] = false;
        }
    }
    unsigned long long m[4];
    int tot = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        m[b] = __ballot(p[b]);
        tot += __popcll(m[b]);
    }
    if (tot == 0) return;                                  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(&e.count[0], (unsigned long long)tot);
    base = __shfl(base, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (p[b]) {
            const long long idx = (long long)base + __popcll(m[b] & below);
            if (idx < e.cap) e.out[idx] = sc[b];
        }
        base += __popcll(m[b]);
    }
}

// TK_CNT: row r's four pairs of one super-block; allneg: the item's boxes are so far apart that every pair is negative
__device__ __forceinline__ void ev_cnt_push(EvalArgs& e, const float (&s)[4], int c0, int M, bool live, int r, double px,
                                            double pz, bool allneg) {
    bool neg[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = c0 + b;
        neg[b] = live && c < M && (allneg || ev_class(e, r, c, px, pz) == 0);
        if (neg[b] && ev_bad(s[b])) {
            ++e.nbad;
            neg[b] = false;
        }
    }
    if (!__any(neg[0] || neg[1] || neg[2] || neg[3])) return;
    thr_count4<1>(e.th, s, neg, e.rank2);
}

// ------------------------------------------------------------------ fused mining epilogue (sgpr_score_mine)
// The top-k epilogue (TK > 0) with one more condition on a candidate: the pose class of the pair (classify_pair's
// float64 rule) must be the one asked for, and c != self_r.  MN_NEG keeps class 0 in top-k's order; MN_POS keeps class 1
// lowest score first - it feeds -score to the same descending lists (tk_merge, tk_flush, topk_merge_kernel) and negates
// on the way out (exact).  The row pose is d_row_pose[r], or the column pose of the row's own frame (mine_rowpose_kernel
// writes them, and every wave's four-row box, to the workspace).  Work items are tested as a whole with the evaluation
// epilogues' gap (ev_gap2 against eval_colbox_kernel's chunk boxes): MN_POS skips an item farther than d_pos from every
// row unscored, MN_NEG takes every pair of an item farther than max(d_pos, d_neg) as a negative without per-pair float64.
// Candidates are classified (classify_pose_exact) only once they beat the row's threshold.
constexpr int MN_NEG = 1;
constexpr int MN_POS = 2;

struct MineArgs {
    PairTruth truth;          // pose: the column poses [M][2], d_pos, d_neg
    const double* rpose;      // [R][2] the pose of every row (mine_rowpose_kernel)
    const double* rbox;       // [ceil(R / 4)][4] the box of every wave's four rows (x lo, x hi, z lo, z hi)
    const double* cbox;       // [ncc][4] column chunk boxes (eval_colbox_kernel)
    double lo2, hi2, cut_pos, cut_neg;
};

// (the row poses and boxes live in memory, not in registers: the top-k instances spill already, and a candidate is
//  classified only once it beats its row's threshold)
template <int MINE>
__device__ __forceinline__ bool mn_class_ok(const MineArgs& m, int r, int c, bool allneg) {
    if (MINE == MN_NEG && allneg) return true;
    asm volatile("" : "+v"(r));                        // (keeps the row pose load here: hoisted, it stays live throughout)
    const double px = m.rpose[2 * (size_t)r], pz = m.rpose[2 * (size_t)r + 1];
    return classify_pose_exact(m.truth.pose, c, px, pz, m.truth.d_pos, m.truth.d_neg, m.lo2, m.hi2) == (MINE == MN_POS ? 1 : 0);
}

// tk_push with the pose class of the pair (allneg: every pair of the work item is a negative); c != self_r is part of
// the window (launch_score_mine passes a window of at least 0).  The four columns are first tested against the row's
// threshold as it stands, the survivors are classified in one rolled loop (one copy of the float64 code, not four), and
// the list takes them with the threshold re-tested as it rises.
template <int K, int MINE>
__device__ __forceinline__ void mn_push(const MineArgs& m, const float (&sc)[4], int c0, int M, int ea, int eb, bool live,
                                        int r, bool allneg, float& tv, int& tc, float& thv, int& thc, float* lsv,
                                        int* lsc) {
    unsigned cand = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = c0 + b;
        const float v = MINE == MN_POS ? -sc[b] : sc[b];
        const bool q = live && c < M && (c < ea || c > eb) && v == v && (K == 1 ? tk_beats(v, c, tv, tc) : tk_beats(v, c, thv, thc));
        cand |= q ? 1u << b : 0u;
    }
    if (cand != 0u && !(MINE == MN_NEG && allneg)) {
#pragma unroll 1
        for (int b = 0; b < 4; ++b)
            if (((cand >> b) & 1u) && !mn_class_ok<MINE>(m, r, c0 + b, false)) cand &= ~(1u << b);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = c0 + b;
        const float v = MINE == MN_POS ? -sc[b] : sc[b];
        if constexpr (K == 1) {
            if (((cand >> b) & 1u) && tk_beats(v, c, tv, tc)) {
                tv = v;
                tc = c;
            }
        } else {
            const bool q = ((cand >> b) & 1u) && tk_beats(v, c, thv, thc);
            if (__any(q)) {
                tk_merge<K>(tv, tc, v, c, q, lsv, lsc);
                const int src = (threadIdx.x & 48) + K - 1;
                thv = __shfl(tv, src);
                thc = __shfl(tc, src);
            }
        }
    }
}

// the work items [it0, it1) of one R x M rectangle
// TK = 0: the matrix is stored to score; TK > 0: the scores feed per-row top-TK lists (*tk), nothing is stored; with
// MINE (MN_NEG / MN_POS) the lists take the mined pairs only (*mn);
// TK = TK_ABOVE: one pass of the range selection (*ab), nothing is stored; TK = TK_POS / TK_CNT: the evaluation
// epilogues (*ev), nothing is stored
template <int NI, int VAR, bool CL, int TK = 0, int MINE = 0>
__device__ __forceinline__ void ap_items(const DevWeights& w, const ApConsts& k, const bool fast, int R, int M,
                                         const unsigned short* __restrict__ Ab, const unsigned short* __restrict__ Cb,
                                         const float* __restrict__ ur, const float* __restrict__ prow,
                                         const float* __restrict__ pcol, float* __restrict__ score, int64_t ld,
                                         const int it0, const int it1, const TopkArgs* tk = nullptr,
                                         const AboveArgs* ab = nullptr, EvalArgs* ev = nullptr,
                                         const MineArgs* mn = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const f16x8 w1hi = k.w1hi, w1lo = k.w1lo;
    const float4 b1v = k.b1v, side = k.side;
    const float nl2e = k.nl2e;
    const float nb2 = k.nb2;
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    f16x8 ah[AP_RW], al[AP_RW];
    f32x4 u4[AP_RW];
    int cur_rg = -1, rbase = 0;
    const int nsb = (M + AP_SB - 1) / AP_SB;
    // top-k state (TK > 0): the list entry / best of this lane (row rbase + g), the row's threshold, its eligible columns
    float tv = -INFINITY, thv = -INFINITY;
    int tc = TK_EMPTY, thc = TK_EMPTY, ea = 0, eb = 0;
    __shared__ float tk_sv[TK > 1 ? 4 : 1][64];
    __shared__ int tk_sc[TK > 1 ? 4 : 1][64];
    float* const lsv = tk_sv[TK > 1 ? wave : 0];
    int* const lsc = tk_sc[TK > 1 ? wave : 0];
    // range state (TK_ABOVE): this lane's hits of row rbase + g (pass 1), the row's running / first position (pass 2)
    int acnt = 0;
    long long apos = 0, astart = 0;
    // evaluation state (TK_POS / TK_CNT): the pose of this lane's row rbase + g and the box of the wave's four rows
    double epx = 0.0, epz = 0.0, erb[4] = {0.0, 0.0, 0.0, 0.0};
    for (int it = it0; it < it1; ++it) {
        const int rg = it / ncc, cc = it - rg * ncc;
        if (rg != cur_rg) {
            if constexpr (TK == TK_ABOVE) {
                if (cur_rg >= 0) ab_flush(*ab, cur_rg, ncc, it0, it1, rbase + g, R, acnt, apos, astart);
                const int r = rg * AP_ROWS + wave * AP_RW + g;
                long long s = ab->row0 + (long long)r;
                if (ab->row_self) {
                    s = ab->row_self[min(r, R - 1)];
                    if (ab->pass == 1 && r < R && l15 == 0 && (s < 0 || s >= M)) atomicOr(ab->status, 16);
                }
                tk_bounds(s, ab->window, ab->causal, ea, eb);
                acnt = 0;
                if (ab->pass == 2) apos = astart = ab_start(*ab, rg, ncc, it0, it1, r, R);
            }
            if constexpr (TK > 0) {
                if (cur_rg >= 0) tk_flush<TK, MINE == MN_POS>(*tk, cur_rg, ncc, it0, it1, rbase + g, R, tv, tc);
                tv = thv = -INFINITY;
                tc = thc = TK_EMPTY;
                const int r = rg * AP_ROWS + wave * AP_RW + g;
                long long s = tk->row0 + (long long)r;
                if (tk->row_self) {
                    s = tk->row_self[min(r, R - 1)];
                    if (r < R && l15 == 0 && (s < 0 || s >= M)) atomicOr(tk->status, 16);
                }
                tk_bounds(s, tk->window, tk->causal, ea, eb);
            }
            cur_rg = rg;
            rbase = rg * AP_ROWS + wave * AP_RW;
            if constexpr (TK == TK_POS || TK == TK_CNT) {
                if (ev->truth.pose) {
                    const int r = min(rbase + g, R - 1);
                    epx = ev->truth.pose[2 * ((int64_t)ev->truth.row0 + r)];
                    epz = ev->truth.pose[2 * ((int64_t)ev->truth.row0 + r) + 1];
                    ev_row_box(epx, epz, erb);
                }
            }
#pragma unroll
            for (int rr = 0; rr < AP_RW; ++rr) {
                const int r = min(rbase + rr, R - 1);
                const unsigned short* ap = Ab + ((size_t)r * 2 * 64 + lane) * 8;      // A'_r[t = l15][8g .. 8g+7]
                ah[rr] = *reinterpret_cast<const f16x8*>(ap);
                al[rr] = *reinterpret_cast<const f16x8*>(ap + 64 * 8);
                const float4 u = *reinterpret_cast<const float4*>(ur + (size_t)r * T + 4 * g);
                u4[rr] = f32x4{u.x, u.y, u.z, u.w};
            }
        }
        const int sb0 = cc * (AP_COLS / AP_SB), sb1 = min(nsb, sb0 + AP_COLS / AP_SB);
        if (rbase >= R) continue;                          // this wave's rows lie past the matrix edge
        if constexpr (TK > 0) {
            // causal without a row_self table: a work item whose first column is ineligible for the last row of the row
            // group (the largest own frame) has no eligible column for any row of it
            if (tk->causal && !tk->row_self) {
                const long long smax = tk->row0 + (long long)min(R, (rg + 1) * AP_ROWS) - 1;
                if ((long long)sb0 * AP_SB >= smax - (tk->window > 0 ? tk->window : 0)) continue;
            }
        }
        if constexpr (TK == TK_ABOVE) {
            // the same skip rule as top-k; pass 2 also skips every work item pass 1 found no hit in
            if (ab->causal && !ab->row_self) {
                const long long smax = ab->row0 + (long long)min(R, (rg + 1) * AP_ROWS) - 1;
                if ((long long)sb0 * AP_SB >= smax - (ab->window > 0 ? ab->window : 0)) continue;
            }
            if (ab->pass == 2 && !ab->flag[it]) continue;
        }
        bool eneg = false;   // TK_CNT / MN_NEG: every pair of this item (and wave) is a negative
        if constexpr (MINE != 0) {
            const double* rb = mn->rbox + 4 * (size_t)(rbase >> 2);
            const double rbv[4] = {rb[0], rb[1], rb[2], rb[3]};
            const double g2 = ev_gap2(rbv, mn->cbox + 4 * (size_t)cc);
            if constexpr (MINE == MN_POS) {
                if (g2 > mn->cut_pos) continue;            // no positive: not even scored
            } else {
                eneg = g2 > mn->cut_neg;
            }
        }
        if constexpr (TK == TK_POS || TK == TK_CNT) {
            if (ev->truth.pose) {
                const double g2 = ev_gap2(erb, ev->cbox + 4 * (size_t)cc);
                if constexpr (TK == TK_POS) {
                    if (g2 > ev->cut_pos) continue;        // no positive: not even scored
                } else {
                    eneg = g2 > ev->cut_neg;
                }
            }
        }
        if (!fast) {      // inputs outside the f16 range: exact fp32 per-pair arithmetic
            if constexpr (TK == 0) {
                slow_tile(w, prow, pcol, rbase, min(R, rbase + AP_RW), sb0 * AP_SB, min(M, sb1 * AP_SB), score, ld);
            } else {
                // the same per-pair values, gathered into the lane layout of the fast path (lane (g, l15): row g,
                // columns 4 l15 .. 4 l15 + 3 of the super-block) and handed to the lists
#pragma unroll 1
                for (int sb = sb0; sb < sb1; ++sb) {
                    float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                    for (int rr = 0; rr < AP_RW && rbase + rr < R; ++rr)
#pragma unroll 1
                        for (int cl = 0; cl < AP_SB && sb * AP_SB + cl < M; ++cl) {
                            // (lane 0's value - the one slow_tile stores -, read into a scalar register: with
                            //  contracted multiply-adds in its shuffle reductions slow_pair's lanes need not agree to
                            //  the last bit; every lane is active here, the loop bounds are wave-uniform)
                            const float v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(
                                slow_pair(w, prow + (size_t)(rbase + rr) * F, pcol + (size_t)(sb * AP_SB + cl) * F))));
                            if (rr == g && (cl >> 2) == l15) {
#pragma unroll
                                for (int b = 0; b < 4; ++b) sc[b] = (cl & 3) == b ? v : sc[b];
                            }
                        }
                    if constexpr (TK == TK_ABOVE)
                        ab_push(*ab, sc, sb * AP_SB + 4 * l15, M, ea, eb, rbase + g < R, rbase + g, it, acnt, apos);
                    else if constexpr (TK == TK_POS)
                        ev_pos_push(*ev, sc, sb * AP_SB + 4 * l15, M, rbase + g < R, rbase + g, epx, epz);
                    else if constexpr (TK == TK_CNT)
                        ev_cnt_push(*ev, sc, sb * AP_SB + 4 * l15, M, rbase + g < R, rbase + g, epx, epz, eneg);
                    else if constexpr (MINE != 0)
                        mn_push<TK, MINE>(*mn, sc, sb * AP_SB + 4 * l15, M, ea, eb, rbase + g < R, rbase + g, eneg, tv,
                                          tc, thv, thc, lsv, lsc);
                    else
                        tk_push<TK>(sc, sb * AP_SB + 4 * l15, M, ea, eb, rbase + g < R, tv, tc, thv, thc, lsv, lsc);
                }
            }
            continue;
        }
        // column operands of block (sb, b): e2_c[8g .. 8g+7], c = 64 sb + 4 l15 + b; 1 KB contiguous per wave and plane,
        // straight from L2 / L1 (the four waves of a workgroup read the same blocks).  Staging them through LDS once per
        // workgroup was measured and is no faster (112 vs 108 us): the kernel is bound by vector issue, not by operands.
        const unsigned short* cp = Cb + (size_t)sb0 * (2 * 4 * 64 * 8) + (size_t)lane * 8;
        f16x8 bh = *reinterpret_cast<const f16x8*>(cp);
        f16x8 bl = *reinterpret_cast<const f16x8*>(cp + 4 * 64 * 8);
        for (int sb = sb0; sb < sb1; ++sb) {
            float zb[4][AP_RW];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                // next block: b + 1 of this super-block, or block 0 of the next one (the last one re-reads itself)
                const int nb = b + 1 < 4 ? b + 1 : 0;
                const int nsbk = b + 1 < 4 ? sb : min(sb + 1, sb1 - 1);
                const unsigned short* np = Cb + ((size_t)nsbk * 2 * 4 + nb) * (64 * 8) + (size_t)lane * 8;
                const f16x8 nbh = (VAR & 4) ? bh : *reinterpret_cast<const f16x8*>(np);
                const f16x8 nbl = (VAR & 4) ? bl : *reinterpret_cast<const f16x8*>(np + 4 * 64 * 8);
#pragma unroll
                for (int r0 = 0; r0 < AP_RW; r0 += NI) {
                    f32x4 h[NI], q[NI];
                    f16x8 hb[NI];
                    if (VAR & 8) __builtin_amdgcn_s_setprio(1);
                    if (VAR & 16) {                      // timing: no matrix instructions (opaque copies keep the vector work alive)
#pragma unroll
                        for (int i = 0; i < NI; ++i) {
                            h[i] = u4[r0 + i];
                            asm volatile("" : "+v"(h[i]) : "v"(bh), "v"(bl));
                        }
                    } else {
#if SGPR_AP_CHAINS == 2
                        f32x4 hc[NI];
#pragma unroll
                        for (int i = 0; i < NI; ++i) hc[i] = mfma_f16(al[r0 + i], bh, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                        for (int i = 0; i < NI; ++i) h[i] = mfma_f16(ah[r0 + i], bh, u4[r0 + i]);
#pragma unroll
                        for (int i = 0; i < NI; ++i) hc[i] = mfma_f16(ah[r0 + i], bl, hc[i]);
#pragma unroll
                        for (int i = 0; i < NI; ++i) h[i] = h[i] + hc[i];
#else
#pragma unroll
                        for (int i = 0; i < NI; ++i) h[i] = mfma_f16(al[r0 + i], bh, u4[r0 + i]);
#pragma unroll
                        for (int i = 0; i < NI; ++i) h[i] = mfma_f16(ah[r0 + i], bl, h[i]);
#pragma unroll
                        for (int i = 0; i < NI; ++i) h[i] = mfma_f16(ah[r0 + i], bh, h[i]);
#endif
                    }
                    if (VAR & 8) __builtin_amdgcn_s_setprio(0);
#pragma unroll
                    for (int i = 0; i < NI; ++i) hb[i] = (VAR & 32) ? __builtin_bit_cast(f16x8, h[i]) : split_relu4<CL>(h[i]);
                    if (VAR & 8) __builtin_amdgcn_s_setprio(1);
                    if (VAR & 16) {
#pragma unroll
                        for (int i = 0; i < NI; ++i) {
                            q[i] = f32x4{b1v.x, b1v.y, b1v.z, b1v.w};
                            asm volatile("" : "+v"(q[i]) : "v"(hb[i]));
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NI; ++i) q[i] = mfma_f16(w1lo, hb[i], f32x4{b1v.x, b1v.y, b1v.z, b1v.w});   // hi . W1lo
#pragma unroll
                        for (int i = 0; i < NI; ++i) q[i] = mfma_f16(w1hi, hb[i], q[i]);                                 // (hi + lo) . W1hi
                    }
                    if (VAR & 8) __builtin_amdgcn_s_setprio(0);
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        if (VAR & 32) {
                            zb[b][r0 + i] = q[i][0];
                            continue;
                        }
                        const float t0 = __builtin_amdgcn_fmed3f(q[i][0], 0.f, side.x), t1 = __builtin_amdgcn_fmed3f(q[i][1], 0.f, side.y);
                        const float t2 = __builtin_amdgcn_fmed3f(q[i][2], 0.f, side.z), t3 = __builtin_amdgcn_fmed3f(q[i][3], 0.f, side.w);
                        zb[b][r0 + i] = (t0 + t1) + (t2 + t3);           // partial over o = 4g..4g+3 of row r0+i, column 4 l15 + b
                    }
                }
                bh = nbh;
                bl = nbl;
            }
            // transpose-reduce over the four lane groups with the gfx950 lane-swap ops: lane group g ends up with the
            // full sum of row g (3 swaps + 3 adds per column block instead of 8 bpermutes), for its 4 columns
            float sc[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float p02 = swap32_add(zb[b][0], zb[b][2]);    // lanes 0-31: row 0 over groups {g, g+2}; 32-63: row 2
                const float p13 = swap32_add(zb[b][1], zb[b][3]);    // likewise rows 1 / 3
                const float zsel = swap16_add(p02, p13);             // even 16-lane rows: row 0 / 2, odd: row 1 / 3
                // sigmoid: v_exp_f32 / v_rcp_f32 (1 ulp each) - far inside the 1e-4 score tolerance
                sc[b] = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(zsel, nl2e, nb2)));
            }
            const int r = rbase + g, c0 = sb * AP_SB + 4 * l15;
            if constexpr (TK > 0 && MINE != 0) {
                mn_push<TK, MINE>(*mn, sc, c0, M, ea, eb, r < R, r, eneg, tv, tc, thv, thc, lsv, lsc);
                continue;
            }
            if constexpr (TK > 0) {
                tk_push<TK>(sc, c0, M, ea, eb, r < R, tv, tc, thv, thc, lsv, lsc);
                continue;
            }
            if constexpr (TK == TK_ABOVE) {
                ab_push(*ab, sc, c0, M, ea, eb, r < R, r, it, acnt, apos);
                continue;
            }
            if constexpr (TK == TK_POS) {
                ev_pos_push(*ev, sc, c0, M, r < R, r, epx, epz);
                continue;
            }
            if constexpr (TK == TK_CNT) {
                ev_cnt_push(*ev, sc, c0, M, r < R, r, epx, epz, eneg);
                continue;
            }
            if ((VAR & 2) && sc[0] + sc[1] + sc[2] + sc[3] != 12345.678f) continue;
            if (r < R) {
                float* dst = score + (size_t)r * ld + c0;
                if (c0 + 3 < M) {
                    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
#if SGPR_AP_NT_STORE
                    __builtin_nontemporal_store(f32x4u{sc[0], sc[1], sc[2], sc[3]}, reinterpret_cast<f32x4u*>(dst));
#else
                    *reinterpret_cast<f32x4u*>(dst) = f32x4u{sc[0], sc[1], sc[2], sc[3]};
#endif
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (c0 + b < M) dst[b] = sc[b];
                }
            }
        }
    }
    if constexpr (TK > 0) {
        if (cur_rg >= 0) tk_flush<TK, MINE == MN_POS>(*tk, cur_rg, ncc, it0, it1, rbase + g, R, tv, tc);
    }
    if constexpr (TK == TK_ABOVE) {
        if (cur_rg >= 0) ab_flush(*ab, cur_rg, ncc, it0, it1, rbase + g, R, acnt, apos, astart);
    }
}

template <int OCC, int NI, int VAR>
__global__ __launch_bounds__(256, OCC) void score_all_pairs_kernel(const DevWeights w, int R, int M,
                                                              const unsigned short* __restrict__ Ab,
                                                              const unsigned short* __restrict__ Cb,
                                                              const float* __restrict__ ur,
                                                              const float* __restrict__ rng, int nrng,
                                                              const float* __restrict__ prow,
                                                              const float* __restrict__ pcol,
                                                              float* __restrict__ score, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    // ---- can every f16 this launch forms be represented?  |A'|, |e2| and |H| <= |u| + 32 max|A'| max|e2|
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, l15, g);
    // work items = (row group of AP_ROWS, column chunk of AP_COLS), row-major; every workgroup takes a contiguous,
    // equally long range (the grid is sized to one resident slot per workgroup, so there is no second,
    // under-occupied round) and reloads its row operands only when the row group changes
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    // workgroups go to the 8 XCDs round-robin and every XCD has its own L2: the workgroups of ONE XCD take neighbouring
    // ranges, so that a row group's A' operands (shared by the ~4 workgroups that split its column chunks) are fetched
    // through one L2 instead of four (FETCH_SIZE 37 -> see profiles)
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    if (mode == 2)
        ap_items<NI, VAR, true>(w, k, true, R, M, Ab, Cb, ur, prow, pcol, score, ld, it0, it1);
    else
        ap_items<NI, VAR, false>(w, k, mode != 0, R, M, Ab, Cb, ur, prow, pcol, score, ld, it0, it1);
}

// the same for several rectangles: the work items of all jobs form one row-major list that the workgroups split evenly
template <int OCC, int NI>
__global__ __launch_bounds__(256, OCC) void score_all_pairs_multi_kernel(const DevWeights w, const ApJobs jobs) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const ApConsts k = ap_consts(w, l15, g);
    const int64_t items = jobs.item0[jobs.n];
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int g0 = (int)(items * wg / nwg), g1 = (int)(items * (wg + 1) / nwg);
#pragma unroll 1
    for (int j = 0; j < jobs.n; ++j) {
        const int lo = max(g0, jobs.item0[j]) - jobs.item0[j], hi = min(g1, jobs.item0[j + 1]) - jobs.item0[j];
        if (lo >= hi) continue;
        const ApJob& q = jobs.job[j];
        float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;        // the f16 range question is answered per rectangle, like
        ap_range(q.rng, q.nrng, am, um, em, l1);             // a call of its own would
        const int mode = ap_mode(am, um, em, l1);
        if (mode == 2)
            ap_items<NI, 0, true>(w, k, true, q.R, q.M, q.Ab, q.Cb, q.ur, q.rows, q.cols, q.score, q.ld, lo, hi);
        else
            ap_items<NI, 0, false>(w, k, mode != 0, q.R, q.M, q.Ab, q.Cb, q.ur, q.rows, q.cols, q.score, q.ld, lo, hi);
    }
}

// the rectangle's top-K per row (sgpr_score_topk): score_all_pairs_kernel's range question, work split and arithmetic,
// the TK epilogue of ap_items instead of the store
#ifndef SGPR_TK_OCC
#define SGPR_TK_OCC 3        // (at four workgroups per CU the k = 1 instance spills 356 bytes per lane, at three nothing)
#endif
constexpr int TK_OCC = SGPR_TK_OCC;

template <int OCC, int NI, int K>
__global__ __launch_bounds__(256, OCC) void score_topk_kernel(const DevWeights w, int R, int M,
                                                              const unsigned short* __restrict__ Ab,
                                                              const unsigned short* __restrict__ Cb,
                                                              const float* __restrict__ ur,
                                                              const float* __restrict__ rng, int nrng,
                                                              const float* __restrict__ prow,
                                                              const float* __restrict__ pcol, TopkArgs a) {
    // (this prologue - range question, ap_consts, XCD-swizzled item range - recurs word for word in score_mine_kernel,
    //  score_above_kernel and score_positives_kernel.  Moved into a __forceinline__ helper with its statement order kept,
    //  it still changes their register allocation and scratch, so each kernel keeps its own copy.)
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, l15, g);
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    a.wg = (int)wg;
    if (mode == 2)
        ap_items<NI, 0, true, K>(w, k, true, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, &a);
    else
        ap_items<NI, 0, false, K>(w, k, mode != 0, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, &a);
}

// the rectangle's mined pairs per row (sgpr_score_mine): score_topk_kernel with the mining conditions (MINE).  At
// three workgroups per CU (top-k's) the float64 pair test spills 36 - 100 bytes per lane more than top-k's instance of
// the same K; at two it spills nothing.
#ifndef SGPR_MN_OCC
#define SGPR_MN_OCC 2
#endif
constexpr int MN_OCC = SGPR_MN_OCC;

template <int OCC, int NI, int K, int MINE>
__global__ __launch_bounds__(256, OCC) void score_mine_kernel(const DevWeights w, int R, int M,
                                                              const unsigned short* __restrict__ Ab,
                                                              const unsigned short* __restrict__ Cb,
                                                              const float* __restrict__ ur,
                                                              const float* __restrict__ rng, int nrng,
                                                              const float* __restrict__ prow,
                                                              const float* __restrict__ pcol, TopkArgs a, MineArgs m) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, l15, g);
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    a.wg = (int)wg;
    if (mode == 2)
        ap_items<NI, 0, true, K, MINE>(w, k, true, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, &a, nullptr, nullptr,
                                       &m);
    else
        ap_items<NI, 0, false, K, MINE>(w, k, mode != 0, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, &a, nullptr,
                                        nullptr, &m);
}

// row groups shared by several workgroups: their partial lists -> the result.  One workgroup per row group, lane group g
// of wave v: row 16 rg + 4 v + g.  The workgroups that touched row group rg are a contiguous run of logical indices.
template <int K, bool NEG = false>
__global__ __launch_bounds__(256) void topk_merge_kernel(int R, int M, int nwg, TopkArgs a) {
    __shared__ float sv[4][64];
    __shared__ int sc[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15;
    const int rg = blockIdx.x;
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const int64_t lo = (int64_t)rg * ncc, hi = lo + ncc;
    int w0 = 0, w1 = nwg - 1;                           // first workgroup whose range ends past lo
    for (int n = nwg - 1; w0 < n;) {
        const int m = (w0 + n) >> 1;
        if (items * (m + 1) / nwg > lo) n = m; else w0 = m + 1;
    }
    for (int n = 0; n < w1;) {                          // last workgroup whose range starts before hi
        const int m = (n + w1 + 1) >> 1;
        if (items * m / nwg < hi) n = m; else w1 = m - 1;
    }
    if (w0 >= w1) return;                               // one workgroup saw the whole row group: its lists are the result
    const int rr = wave * AP_RW + (lane >> 4), r = rg * AP_ROWS + rr;
    float tv = -INFINITY;
    int tc = TK_EMPTY;
#pragma unroll 1
    for (int wv = w0; wv <= w1; ++wv) {
        const int slot = (items * wv / nwg) / ncc == rg ? 0 : 1;
        const size_t p = ((size_t)(wv * 2 + slot) * AP_ROWS + rr) * a.k + l15;
        const bool ok = r < R && l15 < a.k;
        const float cv = ok ? a.pval[p] : -INFINITY;
        const int cc = ok ? a.pidx[p] : TK_EMPTY;
        tk_merge<K>(tv, tc, cv, cc, ok && cc != TK_EMPTY, sv[wave], sc[wave]);
    }
    if (r < R && l15 < a.k) {
        a.val[(size_t)r * a.k + l15] = NEG ? -tv : tv;
        a.idx[(size_t)r * a.k + l15] = tc == TK_EMPTY ? -1 : tc;
    }
}

__global__ __launch_bounds__(256) void topk_fill_kernel(int64_t n, float* __restrict__ val, int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        val[i] = -INFINITY;
        idx[i] = -1;
    }
}

// one pass (a.pass) of the rectangle's range selection (sgpr_score_above): score_topk_kernel with the TK_ABOVE epilogue
template <int OCC, int NI>
__global__ __launch_bounds__(256, OCC) void score_above_kernel(const DevWeights w, int R, int M,
                                                               const unsigned short* __restrict__ Ab,
                                                               const unsigned short* __restrict__ Cb,
                                                               const float* __restrict__ ur,
                                                               const float* __restrict__ rng, int nrng,
                                                               const float* __restrict__ prow,
                                                               const float* __restrict__ pcol, AboveArgs a) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, l15, g);
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    a.wg = (int)wg;
    if (mode == 2)
        ap_items<NI, 0, true, TK_ABOVE>(w, k, true, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, nullptr, &a);
    else
        ap_items<NI, 0, false, TK_ABOVE>(w, k, mode != 0, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, nullptr, &a);
}

// rows of the row groups shared by several workgroups: the partial counts -> cnt[r], and each share's offset within its
// row -> poff (in logical workgroup order = column order).  One wave per row group (topk_merge_kernel's run arithmetic).
__global__ __launch_bounds__(64) void above_fold_kernel(int R, int M, int nwg, AboveArgs a) {
    const int rg = blockIdx.x, rr = threadIdx.x;
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const int64_t lo = (int64_t)rg * ncc, hi = lo + ncc;
    int w0 = 0, w1 = nwg - 1;                           // first workgroup whose range ends past lo
    for (int n = nwg - 1; w0 < n;) {
        const int m = (w0 + n) >> 1;
        if (items * (m + 1) / nwg > lo) n = m; else w0 = m + 1;
    }
    for (int n = 0; n < w1;) {                          // last workgroup whose range starts before hi
        const int m = (n + w1 + 1) >> 1;
        if (items * m / nwg < hi) n = m; else w1 = m - 1;
    }
    const int r = rg * AP_ROWS + rr;
    if (w0 >= w1 || rr >= AP_ROWS || r >= R) return;   // one workgroup saw the whole row group: cnt is final
    int sum = 0;
#pragma unroll 1
    for (int wv = w0; wv <= w1; ++wv) {
        const size_t p = (size_t)(wv * 2 + ((items * wv / nwg) / ncc == rg ? 0 : 1)) * AP_ROWS + rr;
        a.poff[p] = sum;
        sum += a.pcnt[p];
    }
    a.cnt[r] = sum;
}

// cnt [R] -> row_ptr [R + 1] (exclusive, int64) and *count = the total; accumulate: both start from *count (the row
// blocks of the chunked path), else from 0.  One workgroup: each thread adds a contiguous run of rows, the runs' sums are
// scanned across the workgroup, then each thread writes its run.
__global__ __launch_bounds__(1024) void above_scan_kernel(const int32_t* __restrict__ cnt, int R, int64_t* __restrict__ row_ptr,
                                                          unsigned long long* __restrict__ count, int accumulate) {
    __shared__ long long wsum[16];
    __shared__ long long sbase;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (R + 1023) / 1024;
    const int lo = (int)min((int64_t)R, (int64_t)t * per), hi = min(R, lo + per);
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    long long x = s;                                    // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    if (t == 0) sbase = accumulate ? (long long)*count : 0;
    __syncthreads();
    long long run = sbase + x - s;
    for (int v = 0; v < wave; ++v) run += wsum[v];
    for (int i = lo; i < hi; ++i) {
        row_ptr[i] = run;
        run += cnt[i];
    }
    if (t == 0) {
        long long total = sbase;
        for (int v = 0; v < 16; ++v) total += wsum[v];
        row_ptr[R] = total;
        *count = (unsigned long long)total;
    }
}

// the range selection on a resident matrix (sgpr_rows_above and the chunked path): one wave per row.  PASS 1 counts the
// row's hits into cnt[r]; PASS 2 writes them in column order from row_ptr[r] (64 columns per ballot) to output row
// rout0 + r, below cap, and checks the count (status bit 32)
template <int PASS>
__global__ __launch_bounds__(256) void rows_above_kernel(const float* __restrict__ score, int R, int M, int64_t ld,
                                                         const int32_t* __restrict__ row_self, int row0, int window,
                                                         int causal, float thr, int32_t* __restrict__ cnt,
                                                         const int64_t* __restrict__ row_ptr, int rout0,
                                                         int32_t* __restrict__ orows, int32_t* __restrict__ ocols,
                                                         float* __restrict__ ovals, int64_t cap, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    long long s = row0 + (long long)r;
    if (row_self) {
        s = row_self[r];
        if (PASS == 1 && lane == 0 && (s < 0 || s >= M)) atomicOr(status, 16);
    }
    int ea, eb;
    tk_bounds(s, window, causal, ea, eb);
    const int cend = eb == 0x7fffffff ? min(M, max(ea, 0)) : M;    // nothing at or beyond ea is eligible then
    const float* sp = score + (size_t)r * ld;
    if constexpr (PASS == 1) {
        int n = 0;
        for (int c = lane; c < cend; c += 64) n += ((c < ea || c > eb) && sp[c] >= thr) ? 1 : 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
        if (lane == 0) cnt[r] = n;
    } else {
        const long long start = row_ptr[r];
        long long pos = start;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int c0 = 0; c0 < cend; c0 += 64) {
            const int c = c0 + lane;
            const float v = c < cend ? sp[c] : 0.f;
            const bool h = c < cend && (c < ea || c > eb) && v >= thr;
            const unsigned long long B = __ballot(h);
            const long long p = pos + __popcll(B & below);
            if (h && p < cap) {
                orows[p] = rout0 + r;
                ocols[p] = c;
                ovals[p] = v;
            }
            pos += __popcll(B);
        }
        if (lane == 0 && pos - start != cnt[r]) atomicOr(status, 32);
    }
}

// ------------------------------------------------------------------ dense all-pairs at the reference's operand width
// The same rectangle with every matrix operand as THREE bf16 planes (x = hi + mid + lo exactly: 24 bits, fp32's range) on
// v_mfma_f32_16x16x32_bf16 - the tail of layers_batch.py:70-83 / sg_net.py:131-136 at fp32's own operand width, as the
// embed kernel's wide-range instance is for dgcnn_conv_pass.  Selected per handle (weights outside the f16 range) or by
// debug bit 13, never by the data (out-of-range data keeps the exact per-pair path of score_all_pairs_kernel).
// A launch whose range partials are not finite - a NaN or an infinity among A', u or e2 (range_max) - is scored again by
// score_all_pairs_exact_kernel behind this one: the plane cuts, the signed-integer ReLU and the v_med3_f32 of the head
// below do not hand a NaN on (measured: a NaN graph scored like H = 0), and this kernel has no registers left for a
// per-pair path of its own (156 of its 168).
//   layer 1  six significant cross products (lo.hi, hi.lo, mid.mid, mid.hi, hi.mid in a chain of their own - smallest
//            first, never against the large accumulator -, then hi.hi on u_r), one vector add
//   layer 2  H = relu(.) cut into three planes by truncation (upper halves of x, x - hi, x - hi - mid: same sign, so the
//            ReLU is a signed maximum of the fp32 word before the cut); the eight K slots of a lane group carry two planes
//            per instruction: [Hh | Hm].[W1h | W1h], [Hl | Hh].[W1h | W1m], [Hm | Hh].[W1m | W1l] - again six products
// Everything else (u_r, the folded head, the lane-swap transpose-reduce, 16-byte stores, the work split) is the f16
// instance's.  Nine matrix instructions and ~45 vector instructions per (row, 16 columns) against five and ~24.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// {upper half of b, upper half of a} -> one dword: K slot 2i in the low half, 2i + 1 in the high half
__device__ __forceinline__ unsigned pack_hi16(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

#ifndef SGPR_APW_OCC
#define SGPR_APW_OCC 3
#endif
#ifndef SGPR_APW_NI
#define SGPR_APW_NI 1         // (2: same time, same box - 226.9 / 230.1 against 226.9 / 226.5 us - and 12 registers more)
#endif
constexpr int APW_NI = SGPR_APW_NI;       // row graphs interleaved in program order (1, 2 or 4)
constexpr int APW_OCC = SGPR_APW_OCC;     // (three row-operand planes of four row graphs: 48 registers; three workgroups per CU)

__global__ __launch_bounds__(256, APW_OCC) void score_all_pairs_wide_kernel(const DevWeights w, int R, int M,
                                                                            const unsigned short* __restrict__ Ab,
                                                                            const unsigned short* __restrict__ Cb,
                                                                            const float* __restrict__ ur,
                                                                            float* __restrict__ score, int64_t ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    // the head folded into layer 2 (ap_consts), W1 as three planes in the three slot arrangements
    bf16x8 wa, wb2, wc;
    float4 b1v, side;
    {
        const float s = w.fc2_w[l15];
        const float4 w1 = *reinterpret_cast<const float4*>(w.fc1_w + l15 * T + 4 * g);
        const float v[4] = {s * w1.x, s * w1.y, s * w1.z, s * w1.w};
        unsigned hb[4], mb[4], lb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split3_bf16(v[i], hb[i], mb[i], lb[i]);
        const unsigned h01 = pack_hi16(hb[0], hb[1]), h23 = pack_hi16(hb[2], hb[3]);
        const unsigned m01 = pack_hi16(mb[0], mb[1]), m23 = pack_hi16(mb[2], mb[3]);
        const unsigned l01 = pack_hi16(lb[0], lb[1]), l23 = pack_hi16(lb[2], lb[3]);
        wa = __builtin_bit_cast(bf16x8, u32x4{h01, h23, h01, h23});
        wb2 = __builtin_bit_cast(bf16x8, u32x4{h01, h23, m01, m23});
        wc = __builtin_bit_cast(bf16x8, u32x4{m01, m23, l01, l23});
        const float4 b1 = *reinterpret_cast<const float4*>(w.fc1_b + 4 * g);
        const float4 w2 = *reinterpret_cast<const float4*>(w.fc2_w + 4 * g);
        b1v = make_float4(w2.x * b1.x, w2.y * b1.y, w2.z * b1.z, w2.w * b1.w);
        side = make_float4(w2.x < 0.f ? -INFINITY : INFINITY, w2.y < 0.f ? -INFINITY : INFINITY,
                           w2.z < 0.f ? -INFINITY : INFINITY, w2.w < 0.f ? -INFINITY : INFINITY);
    }
    const float kL2E = 1.4426950408889634f;
    const float nb2 = -w.fc2_b[0] * kL2E;
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    const int nsb = (M + AP_SB - 1) / AP_SB;
    bf16x8 ah[AP_RW], am[AP_RW], al[AP_RW];
    f32x4 u4[AP_RW];
    int cur_rg = -1, rbase = 0;
    for (int it = it0; it < it1; ++it) {
        const int rg = it / ncc, cc = it - rg * ncc;
        if (rg != cur_rg) {
            cur_rg = rg;
            rbase = rg * AP_ROWS + wave * AP_RW;
#pragma unroll
            for (int rr = 0; rr < AP_RW; ++rr) {
                const int r = min(rbase + rr, R - 1);
                const unsigned short* ap = Ab + ((size_t)r * 3 * 64 + lane) * 8;      // A'_r[t = l15][8g .. 8g+7]
                ah[rr] = *reinterpret_cast<const bf16x8*>(ap);
                am[rr] = *reinterpret_cast<const bf16x8*>(ap + 64 * 8);
                al[rr] = *reinterpret_cast<const bf16x8*>(ap + 2 * 64 * 8);
                const float4 u = *reinterpret_cast<const float4*>(ur + (size_t)r * T + 4 * g);
                u4[rr] = f32x4{u.x, u.y, u.z, u.w};
            }
        }
        const int sb0 = cc * (AP_COLS / AP_SB), sb1 = min(nsb, sb0 + AP_COLS / AP_SB);
        if (rbase >= R) continue;                          // this wave's rows lie past the matrix edge
        const unsigned short* cp = Cb + (size_t)sb0 * (3 * 4 * 64 * 8) + (size_t)lane * 8;
        bf16x8 bh = *reinterpret_cast<const bf16x8*>(cp);
        bf16x8 bm = *reinterpret_cast<const bf16x8*>(cp + 4 * 64 * 8);
        bf16x8 bl = *reinterpret_cast<const bf16x8*>(cp + 2 * 4 * 64 * 8);
        for (int sb = sb0; sb < sb1; ++sb) {
            float zb[4][AP_RW];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int nb = b + 1 < 4 ? b + 1 : 0;
                const int nsbk = b + 1 < 4 ? sb : min(sb + 1, sb1 - 1);
                const unsigned short* np = Cb + ((size_t)nsbk * 3 * 4 + nb) * (64 * 8) + (size_t)lane * 8;
                const bf16x8 nbh = *reinterpret_cast<const bf16x8*>(np);
                const bf16x8 nbm = *reinterpret_cast<const bf16x8*>(np + 4 * 64 * 8);
                const bf16x8 nbl = *reinterpret_cast<const bf16x8*>(np + 2 * 4 * 64 * 8);
#pragma unroll
                for (int r0 = 0; r0 < AP_RW; r0 += APW_NI) {
                    // APW_NI row graphs interleaved in program order: their dependent MFMA -> vector -> MFMA chains overlap
                    f32x4 c[APW_NI], h[APW_NI], qc[APW_NI], q[APW_NI];
                    unsigned h01[APW_NI], h23[APW_NI], m01[APW_NI], m23[APW_NI], l01[APW_NI], l23[APW_NI];
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) c[i] = mfma_bf16(al[r0 + i], bh, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) h[i] = mfma_bf16(ah[r0 + i], bh, u4[r0 + i]);
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) c[i] = mfma_bf16(ah[r0 + i], bl, c[i]);
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) c[i] = mfma_bf16(am[r0 + i], bm, c[i]);
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) c[i] = mfma_bf16(am[r0 + i], bh, c[i]);
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) c[i] = mfma_bf16(ah[r0 + i], bm, c[i]);
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) {
                        h[i] = h[i] + c[i];
                        // relu, then the three planes of each of the lane's four values (t = 4g .. 4g+3)
                        unsigned hb[4], mb[4], lb[4];
#pragma unroll
                        for (int v = 0; v < 4; ++v) split3_bf16(relu(h[i][v]), hb[v], mb[v], lb[v]);
                        h01[i] = pack_hi16(hb[0], hb[1]);
                        h23[i] = pack_hi16(hb[2], hb[3]);
                        m01[i] = pack_hi16(mb[0], mb[1]);
                        m23[i] = pack_hi16(mb[2], mb[3]);
                        l01[i] = pack_hi16(lb[0], lb[1]);
                        l23[i] = pack_hi16(lb[2], lb[3]);
                    }
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i)                                                       // Hm.W1m + Hh.W1l
                        qc[i] = mfma_bf16(wc, __builtin_bit_cast(bf16x8, u32x4{m01[i], m23[i], h01[i], h23[i]}), f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i)                                                       // Hh.W1h + Hm.W1h
                        q[i] = mfma_bf16(wa, __builtin_bit_cast(bf16x8, u32x4{h01[i], h23[i], m01[i], m23[i]}), f32x4{b1v.x, b1v.y, b1v.z, b1v.w});
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i)                                                       // Hl.W1h + Hh.W1m
                        qc[i] = mfma_bf16(wb2, __builtin_bit_cast(bf16x8, u32x4{l01[i], l23[i], h01[i], h23[i]}), qc[i]);
#pragma unroll
                    for (int i = 0; i < APW_NI; ++i) {
                        q[i] = q[i] + qc[i];
                        const float t0 = __builtin_amdgcn_fmed3f(q[i][0], 0.f, side.x), t1 = __builtin_amdgcn_fmed3f(q[i][1], 0.f, side.y);
                        const float t2 = __builtin_amdgcn_fmed3f(q[i][2], 0.f, side.z), t3 = __builtin_amdgcn_fmed3f(q[i][3], 0.f, side.w);
                        zb[b][r0 + i] = (t0 + t1) + (t2 + t3);
                    }
                }
                bh = nbh;
                bm = nbm;
                bl = nbl;
            }
            float sc[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float p02 = swap32_add(zb[b][0], zb[b][2]);
                const float p13 = swap32_add(zb[b][1], zb[b][3]);
                const float zsel = swap16_add(p02, p13);
                sc[b] = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(zsel, -kL2E, nb2)));
            }
            const int r = rbase + g, c0 = sb * AP_SB + 4 * l15;
            if (r < R) {
                float* dst = score + (size_t)r * ld + c0;
                if (c0 + 3 < M) {
                    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
                    *reinterpret_cast<f32x4u*>(dst) = f32x4u{sc[0], sc[1], sc[2], sc[3]};
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (c0 + b < M) dst[b] = sc[b];
                }
            }
        }
    }
}

// Behind score_all_pairs_wide_kernel, on the same stream: nothing unless a range partial of the launch is not finite (a
// NaN, which range_max turns into +infinity, or an infinity among A', u or e2); then the whole rectangle again in exact
// fp32 per-pair arithmetic, which keeps a NaN (slow_pair) - the work items of the tails, AP_RW rows of a wave x AP_COLS
// columns, grid-strided.
__global__ __launch_bounds__(256) void score_all_pairs_exact_kernel(const DevWeights w, int R, int M,
                                                                    const float* __restrict__ rng, int nrng,
                                                                    const float* __restrict__ prow,
                                                                    const float* __restrict__ pcol,
                                                                    float* __restrict__ score, int64_t ld) {
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    if (am < INFINITY && um < INFINITY && em < INFINITY) return;
    const int wave = threadIdx.x >> 6;
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int rg = (int)(it / ncc), cc = (int)(it - (int64_t)rg * ncc);
        const int rbase = rg * AP_ROWS + wave * AP_RW;
        if (rbase >= R) continue;
        slow_tile(w, prow, pcol, rbase, min(R, rbase + AP_RW), cc * AP_COLS, min(M, (cc + 1) * AP_COLS), score, ld);
    }
}

// ntn_prep_kernel: the two-plane operands of the R x M rectangle into o, nrng prep workgroups
static int launch_ntn_prep(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, const ApOperands& o,
                           int nrng, hipStream_t stream) {
    hipLaunchKernelGGL(ntn_prep_kernel, dim3(nrng), dim3(256), 0, stream, h->w, rows, R, cols, M, o.Ab, o.ur, o.rng, o.Cb);
    return launched("ntn_prep_kernel launch");
}

// one call's range partials folded into g (a float4, max with what g holds): its launches then read g alone (nrng = 1)
__global__ __launch_bounds__(256) void ap_range_fold_kernel(const float* __restrict__ rng, int nrng, float* __restrict__ g) {
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    if (threadIdx.x == 0)
        *reinterpret_cast<float4*>(g) = make_float4(fmaxf(g[0], am), fmaxf(g[1], um), fmaxf(g[2], em), fmaxf(g[3], l1));
}

// The f16-range question of a call that scores R rows in blocks of rb, answered once over the whole rectangle: a first
// pass preps every block into the operand region ws (the block's launch preps it again) and folds its partials into g, so
// that every block takes the datapath sgpr_score_all_pairs takes on the same rectangle.
int launch_call_range(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, int rb, void* ws, float* g,
                      hipStream_t stream) {
    hipError_t e = hipMemsetAsync(g, 0, 4 * sizeof(float), stream);
    if (e != hipSuccess) return hip_fail(e, "call range: clearing");
    for (int r0 = 0; r0 < R; r0 += rb) {
        const int n = R - r0 < rb ? R - r0 : rb;
        const int nrng = 2 * ap_prep_groups(n, M);
        const ApOperands o = ap_operands(ws, n, nrng, 2);
        const int rc = launch_ntn_prep(h, rows + (size_t)r0 * F, n, cols, M, o, nrng, stream);
        if (rc != SGPR_OK) return rc;
        hipLaunchKernelGGL(ap_range_fold_kernel, dim3(1), dim3(256), 0, stream, o.rng, nrng, g);
        if (int rc = launched("ap_range_fold_kernel launch")) return rc;
    }
    return SGPR_OK;
}

int launch_score_all_pairs(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, float* score,
                           int64_t ld, void* ws, hipStream_t stream, bool wide, const float* crng) {
    if (R == 0 || M == 0) return SGPR_OK;
    const int nrng = 2 * ap_prep_groups(R, M);
    const ApOperands o = ap_operands(ws, R, nrng, wide ? 3 : 2);
    const int64_t items = (int64_t)((M + AP_COLS - 1) / AP_COLS) * ((R + AP_ROWS - 1) / AP_ROWS);
    if (wide) {                                            // three bf16 planes: the reference's operand width, fp32's range
        hipLaunchKernelGGL(ntn_prep_wide_kernel, dim3(nrng), dim3(256), 0, stream, h->w, rows, R, cols, M, o.Ab, o.ur, o.rng,
                           o.Cb);
        if (int rc = launched("ntn_prep_wide_kernel launch")) return rc;
        const int64_t slots = (int64_t)h->num_cus * APW_OCC;
        const unsigned grid = (unsigned)(items < slots ? items : slots);
        hipLaunchKernelGGL(score_all_pairs_wide_kernel, dim3(grid), dim3(256), 0, stream, h->w, R, M, o.Ab, o.Cb, o.ur, score,
                           ld);
        if (int rc = launched("score_all_pairs_wide_kernel launch")) return rc;
        const int64_t eslots = (int64_t)h->num_cus * AP_OCC;      // (every workgroup reads the partials, as the f16 tail's do)
        hipLaunchKernelGGL(score_all_pairs_exact_kernel, dim3((unsigned)(items < eslots ? items : eslots)), dim3(256), 0,
                           stream, h->w, R, M, o.rng, nrng, rows, cols, score, ld);
        return launched("score_all_pairs_exact_kernel launch");
    }
    const int rc = launch_ntn_prep(h, rows, R, cols, M, o, nrng, stream);
    if (rc != SGPR_OK) return rc;
    const int64_t slots = (int64_t)h->num_cus * AP_OCC;   // one resident slot per workgroup: a single, full round
    const unsigned grid = (unsigned)(items < slots ? items : slots);
    hipLaunchKernelGGL((score_all_pairs_kernel<AP_OCC, AP_NI, 0>), dim3(grid), dim3(256), 0, stream, h->w, R, M, o.Ab, o.Cb,
                       o.ur, crng ? crng : o.rng, crng ? 1 : nrng, rows, cols, score, ld);
    return launched("score_all_pairs_kernel launch");
}


size_t score_all_pairs_multi_ws_bytes(int n, const sgpr_pairs_job* jobs) {
    size_t total = 0;
    for (int j = 0; j < n; ++j) total += a256(score_all_pairs_ws_bytes(jobs[j].R, jobs[j].M));
    return total;
}

int launch_score_all_pairs_multi(const sgpr_handle* h, int n, const sgpr_pairs_job* jobs, void* ws, hipStream_t stream) {
    ApJobs a;
    memset(&a, 0, sizeof(a));
    unsigned char* base = static_cast<unsigned char*>(ws);
    int64_t items = 0;
    int blocks = 0;
    for (int j = 0; j < n; ++j) {
        const int R = jobs[j].R, M = jobs[j].M;
        if (R == 0 || M == 0) continue;                    // empty rectangles take no work
        ApJob& q = a.job[a.n];
        const int nrng = 2 * ap_prep_groups(R, M);
        q.rows = jobs[j].d_pooled_rows;
        q.cols = jobs[j].d_pooled_cols;
        q.score = jobs[j].d_score;
        q.ld = jobs[j].ld;
        q.R = R;
        q.M = M;
        q.nrng = nrng;
        const ApOperands o = ap_operands(base, R, nrng, 2);   // the layout of launch_score_all_pairs, per job
        q.ur = o.ur;
        q.rng = o.rng;
        q.Ab = o.Ab;
        q.Cb = o.Cb;
        base += a256(score_all_pairs_ws_bytes(R, M));
        a.block0[a.n] = blocks;
        a.item0[a.n] = (int)items;
        blocks += nrng;
        items += (int64_t)((M + AP_COLS - 1) / AP_COLS) * ((R + AP_ROWS - 1) / AP_ROWS);
        if (items > 0x7fffffff) {
            set_error("sgpr_score_all_pairs_multi: more than 2^31 work items");
            return SGPR_E_INVALID;
        }
        ++a.n;
    }
    if (a.n == 0) return SGPR_OK;
    a.block0[a.n] = blocks;
    a.item0[a.n] = (int)items;
    hipLaunchKernelGGL(ntn_prep_multi_kernel, dim3(blocks), dim3(256), 0, stream, h->w, a);
    if (int rc = launched("ntn_prep_multi_kernel launch")) return rc;
    const int64_t slots = (int64_t)h->num_cus * AP_MULTI_OCC;
    const unsigned grid = (unsigned)(items < slots ? items : slots);
    // (one row graph at a time here: at four workgroups per CU interleaving two cost this instance - two instantiations
    //  of the loop in one job loop - 380 -> ~900 bytes of scratch per lane, 334 -> 420 us on the five KITTI matrices; at
    //  three per CU nothing spills either way and the two are on par, 358.9 / 360.8 us: same-box A/Bs, round 5)
    hipLaunchKernelGGL((score_all_pairs_multi_kernel<AP_MULTI_OCC, 1>), dim3(grid), dim3(256), 0, stream, h->w, a);
    return launched("score_all_pairs_multi_kernel launch");
}

// ------------------------------------------------------------------ fused score + top-k (sgpr_score_topk)
// workspace: score_all_pairs' operands | partial lists [grid][2][AP_ROWS][k] values f32 | the same, columns i32
static int64_t topk_grid(const sgpr_handle* h, int R, int M) {
    const int64_t items = (int64_t)((M + AP_COLS - 1) / AP_COLS) * ((R + AP_ROWS - 1) / AP_ROWS);
    const int64_t slots = (int64_t)h->num_cus * TK_OCC;
    return items < slots ? items : slots;
}

size_t score_topk_ws_bytes(const sgpr_handle* h, int R, int M, int k) {
    if (R == 0 || M == 0) return 0;
    const size_t lists = (size_t)topk_grid(h, R, M) * 2 * AP_ROWS * k;
    return a256(score_all_pairs_ws_bytes(R, M)) + a256(lists * sizeof(float)) + lists * sizeof(int32_t);
}

// the list arguments of sgpr_score_topk / sgpr_score_mine: the result, and the partial lists behind the operands
static TopkArgs topk_args(const sgpr_handle* h, int R, int M, const Eligible& e, const ListOut& out, void* ws) {
    const size_t lists = (size_t)topk_grid(h, R, M) * 2 * AP_ROWS * out.k;
    TopkArgs a;
    a.row_self = e.row_self;
    a.row0 = e.row0;
    a.window = e.window;
    a.causal = e.causal;
    a.k = out.k;
    a.wg = 0;
    a.val = out.val;
    a.idx = out.idx;
    a.pval = reinterpret_cast<float*>(static_cast<unsigned char*>(ws) + a256(score_all_pairs_ws_bytes(R, M)));
    a.pidx = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(a.pval) + a256(lists * sizeof(float)));
    a.status = h->d_status;
    return a;
}

int launch_score_topk(const sgpr_handle* h, const PooledRect& p, const Eligible& e, const ListOut& out, void* ws,
                      hipStream_t stream) {
    const int R = p.R, M = p.M, k = out.k;
    const float *rows = p.rows, *cols = p.cols;
    if (R == 0) return SGPR_OK;
    if (M == 0) {                                          // no column at all: every slot is empty
        const int64_t n = (int64_t)R * k;
        hipLaunchKernelGGL(topk_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, out.val, out.idx);
        return launched("topk_fill_kernel launch");
    }
    const int nrng = 2 * ap_prep_groups(R, M);
    const ApOperands o = ap_operands(ws, R, nrng, 2);
    const int64_t grid = topk_grid(h, R, M);
    const TopkArgs a = topk_args(h, R, M, e, out, ws);
    int rc = launch_ntn_prep(h, rows, R, cols, M, o, nrng, stream);
    if (rc != SGPR_OK) return rc;
    const dim3 gd((unsigned)grid), bd(256), gm((unsigned)((R + AP_ROWS - 1) / AP_ROWS));
    rc = launch_list_k(k, "score_topk_kernel launch", [&](auto K) {
        hipLaunchKernelGGL((score_topk_kernel<TK_OCC, AP_NI, K>), gd, bd, 0, stream, h->w, R, M, o.Ab, o.Cb, o.ur, o.rng, nrng,
                           rows, cols, a);
    });
    if (rc != SGPR_OK) return rc;
    return launch_list_k(k, "topk_merge_kernel launch", [&](auto K) {
        hipLaunchKernelGGL((topk_merge_kernel<K>), gm, bd, 0, stream, R, M, (int)grid, a);
    });
}

// ------------------------------------------------------------------ fused score + range selection (sgpr_score_above)
// Rows go in blocks of at most AB_ROWS (the row operands take 2 KB per row: 0.6 GB at 300 k rows in one launch); the
// positions of a block continue from the device-resident count of the blocks before it, and the f16 range is the
// call's (launch_call_range).
// workspace: row_ptr [R + 1] i64 (used when the caller passes none) | for one row block: score_all_pairs' operands |
// flag [items] u8 | cnt [rows] i32 | pcnt, poff [grid][2][AP_ROWS] i32 | (more than one block) the call's range, a float4
constexpr int AB_ROWS = 131072;

static size_t above_block_ws_bytes(const sgpr_handle* h, int R, int M) {
    const size_t items = (size_t)((M + AP_COLS - 1) / AP_COLS) * ((R + AP_ROWS - 1) / AP_ROWS);
    const size_t slots = (size_t)topk_grid(h, R, M) * 2 * AP_ROWS;
    return a256(score_all_pairs_ws_bytes(R, M)) + a256(items) + a256((size_t)R * 4) + 2 * a256(slots * 4);
}

size_t score_above_ws_bytes(const sgpr_handle* h, int R, int M) {
    if (R == 0 || M == 0) return 0;
    return a256((size_t)(R + 1) * 8) + above_block_ws_bytes(h, R < AB_ROWS ? R : AB_ROWS, M) + (R > AB_ROWS ? 256 : 0);
}

size_t rows_above_ws_bytes(int R) { return R == 0 ? 0 : a256((size_t)R * 4) + a256((size_t)(R + 1) * 8); }

int launch_above_empty(int R, int64_t* row_ptr, unsigned long long* count, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), stream);
    if (e == hipSuccess && row_ptr) e = hipMemsetAsync(row_ptr, 0, (size_t)(R + 1) * sizeof(int64_t), stream);
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "sgpr_score_above: clearing the counts");
}

// one row block: rows [out.rout0, out.rout0 + R) of the call; out.row_ptr = the call's row_ptr + out.rout0; crng: the
// call's range (or nullptr: the block is the call, its own partials are)
static int launch_above_block(const sgpr_handle* h, const PooledRect& p, const Eligible& el, float thr, const RangeOut& out,
                              const float* crng, hipStream_t stream) {
    const int R = p.R, M = p.M;
    const float *rows = p.rows, *cols = p.cols;
    void* ws = out.ws;
    const int nrng = 2 * ap_prep_groups(R, M);
    const ApOperands o = ap_operands(ws, R, nrng, 2);
    const float* krng = crng ? crng : o.rng;
    const int knrng = crng ? 1 : nrng;
    const int64_t grid = topk_grid(h, R, M);
    const size_t items = (size_t)((M + AP_COLS - 1) / AP_COLS) * ((R + AP_ROWS - 1) / AP_ROWS);
    const size_t slots = (size_t)grid * 2 * AP_ROWS;
    unsigned char* q = static_cast<unsigned char*>(ws) + a256(score_all_pairs_ws_bytes(R, M));
    AboveArgs a;
    a.row_self = el.row_self;
    a.row0 = el.row0;
    a.window = el.window;
    a.causal = el.causal;
    a.pass = 1;
    a.wg = 0;
    a.thr = thr;
    a.flag = q;
    q += a256(items);
    a.cnt = reinterpret_cast<int32_t*>(q);
    q += a256((size_t)R * 4);
    a.pcnt = reinterpret_cast<int32_t*>(q);
    q += a256(slots * 4);
    a.poff = reinterpret_cast<int32_t*>(q);
    a.rout0 = out.rout0;
    a.row_ptr = out.row_ptr;
    a.rows = out.rows;
    a.cols = out.cols;
    a.vals = out.vals;
    a.cap = out.cap;
    a.status = h->d_status;
    const hipError_t e = hipMemsetAsync(a.flag, 0, items, stream);
    if (e != hipSuccess) return hip_fail(e, "sgpr_score_above: clearing the item flags");
    const int rc = launch_ntn_prep(h, rows, R, cols, M, o, nrng, stream);
    if (rc != SGPR_OK) return rc;
    const dim3 gd((unsigned)grid), bd(256);
    hipLaunchKernelGGL((score_above_kernel<TK_OCC, AP_NI>), gd, bd, 0, stream, h->w, R, M, o.Ab, o.Cb, o.ur, krng, knrng,
                       rows, cols, a);
    if (int rc = launched("score_above_kernel launch (pass 1)")) return rc;
    hipLaunchKernelGGL(above_fold_kernel, dim3((unsigned)((R + AP_ROWS - 1) / AP_ROWS)), dim3(64), 0, stream, R, M, (int)grid, a);
    if (int rc = launched("above_fold_kernel launch")) return rc;
    if (int rc = launch_above_scan(a.cnt, R, out.row_ptr, out.count, out.accumulate, stream)) return rc;
    if (out.cap == 0) return SGPR_OK;                      // count only
    a.pass = 2;
    hipLaunchKernelGGL((score_above_kernel<TK_OCC, AP_NI>), gd, bd, 0, stream, h->w, R, M, o.Ab, o.Cb, o.ur, krng, knrng,
                       rows, cols, a);
    return launched("score_above_kernel launch (pass 2)");
}

int launch_score_above(const sgpr_handle* h, const PooledRect& p, const Eligible& e, float thr, const RangeOut& out,
                       hipStream_t stream) {
    const int R = p.R, M = p.M;
    const float *rows = p.rows, *cols = p.cols;
    if (R == 0 || M == 0) return launch_above_empty(R, out.row_ptr, out.count, stream);
    unsigned char* base = static_cast<unsigned char*>(out.ws);
    RangeOut call = out;
    if (!call.row_ptr) call.row_ptr = reinterpret_cast<int64_t*>(base);
    void* bws = base + a256((size_t)(R + 1) * 8);
    float* crng = nullptr;
    if (R > AB_ROWS) {
        crng = reinterpret_cast<float*>(static_cast<unsigned char*>(bws) + above_block_ws_bytes(h, AB_ROWS, M));
        const int rc = launch_call_range(h, rows, R, cols, M, AB_ROWS, bws, crng, stream);
        if (rc != SGPR_OK) return rc;
    }
    for (int r0 = 0; r0 < R; r0 += AB_ROWS) {
        const int n = R - r0 < AB_ROWS ? R - r0 : AB_ROWS;
        const PooledRect pb = {rows + (size_t)r0 * F, n, cols, M};
        const int rc = launch_above_block(h, pb, e.from(r0), thr, call.at(r0, bws), crng, stream);
        if (rc != SGPR_OK) return rc;
    }
    return SGPR_OK;
}

int launch_above_scan(const int32_t* cnt, int n, int64_t* row_ptr, unsigned long long* count, int accumulate,
                      hipStream_t stream) {
    hipLaunchKernelGGL(above_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, n, row_ptr, count, accumulate);
    return launched("above_scan_kernel launch");
}

int launch_rows_above(const ScoreBlock& b, const Eligible& e, float thr, const RangeOut& out, hipStream_t stream) {
    if (b.R == 0) return SGPR_OK;
    int32_t* cnt = static_cast<int32_t*>(out.ws);
    const dim3 grid((unsigned)((b.R + 3) / 4)), block(256);
    auto pass = [&](auto P, const char* what) {
        hipLaunchKernelGGL(rows_above_kernel<decltype(P)::value>, grid, block, 0, stream, b.score, b.R, b.M, b.ld,
                           e.row_self, e.row0, e.window, e.causal, thr, cnt, out.row_ptr, out.rout0, out.rows, out.cols,
                           out.vals, out.cap, out.status);
        return launched(what);
    };
    if (int rc = pass(std::integral_constant<int, 1>(), "rows_above_kernel launch (pass 1)")) return rc;
    if (int rc = launch_above_scan(cnt, b.R, out.row_ptr, out.count, out.accumulate, stream)) return rc;
    if (out.cap == 0) return SGPR_OK;
    return pass(std::integral_constant<int, 2>(), "rows_above_kernel launch (pass 2)");
}

// ------------------------------------------------------------------ fused evaluation (sgpr_score_positives / sgpr_score_threshold_counts)
// score_topk_kernel's range question, work split and arithmetic with the TK_POS / TK_CNT epilogue.  Rows go in blocks:
// at most AB_ROWS of them, and few enough that no workgroup sees 2^20 work items (4096 pairs each): its 32-bit LDS
// counters cannot overflow; the f16 range is the whole call's (launch_call_range).  workspace: column boxes [ncc][4] f64 |
// slabs [grid][slab words] u32 (counts only) | for one row block: score_all_pairs' operands | (more than one block) the
// call's range, a float4
constexpr int64_t EV_ITEMS_PER_WG = (1 << 20) - 1;

// the pose box of every 256-column chunk: one wave per chunk, four columns per lane (a NaN pose: the whole plane)
__global__ __launch_bounds__(64) void eval_colbox_kernel(const double* __restrict__ pose, int M, double* __restrict__ box) {
    const int cc = blockIdx.x, lane = threadIdx.x;
    double xl = INFINITY, xh = -INFINITY, zl = INFINITY, zh = -INFINITY;
    bool nan = false;
    for (int c = cc * AP_COLS + lane; c < min(M, (cc + 1) * AP_COLS); c += 64) {
        const double x = pose[2 * (size_t)c], z = pose[2 * (size_t)c + 1];
        nan = nan || x != x || z != z;
        xl = fmin(xl, x);
        xh = fmax(xh, x);
        zl = fmin(zl, z);
        zh = fmax(zh, z);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        xl = fmin(xl, __shfl_xor(xl, m));
        xh = fmax(xh, __shfl_xor(xh, m));
        zl = fmin(zl, __shfl_xor(zl, m));
        zh = fmax(zh, __shfl_xor(zh, m));
    }
    if (__any(nan)) {
        xl = zl = -INFINITY;
        xh = zh = INFINITY;
    }
    if (lane == 0) {
        box[4 * (size_t)cc] = xl;
        box[4 * (size_t)cc + 1] = xh;
        box[4 * (size_t)cc + 2] = zl;
        box[4 * (size_t)cc + 3] = zh;
    }
}

template <int OCC, int NI>
__global__ __launch_bounds__(256, OCC) void score_positives_kernel(const DevWeights w, int R, int M,
                                                                   const unsigned short* __restrict__ Ab,
                                                                   const unsigned short* __restrict__ Cb,
                                                                   const float* __restrict__ ur,
                                                                   const float* __restrict__ rng, int nrng,
                                                                   const float* __restrict__ prow,
                                                                   const float* __restrict__ pcol, EvalArgs a) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, l15, g);
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    a.nbad = 0u;
    if (mode == 2)
        ap_items<NI, 0, true, TK_POS>(w, k, true, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, nullptr, nullptr, &a);
    else
        ap_items<NI, 0, false, TK_POS>(w, k, mode != 0, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, nullptr, nullptr, &a);
    unsigned nb = a.nbad;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) nb += __shfl_xor(nb, m);
    if (lane == 0 && nb) atomicAdd(&a.count[1], (unsigned long long)nb);
}

template <int OCC, int NI>
__global__ __launch_bounds__(256, OCC) void score_counts_kernel(const DevWeights w, int R, int M,
                                                                const unsigned short* __restrict__ Ab,
                                                                const unsigned short* __restrict__ Cb,
                                                                const float* __restrict__ ur,
                                                                const float* __restrict__ rng, int nrng,
                                                                const float* __restrict__ prow,
                                                                const float* __restrict__ pcol, EvalArgs a,
                                                                const float* __restrict__ thr,
                                                                const unsigned long long* __restrict__ at_least,
                                                                unsigned* __restrict__ slabs) {
    __shared__ float tree[EV_TP];
    __shared__ unsigned cnt[EV_TP];
    __shared__ unsigned long long atl[EV_MAX_T];
    __shared__ unsigned long long tail[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int l15 = lane & 15, g = lane >> 4;
    ThrView& t = a.th;
    thr_build_tree(tree, thr_levels(t.T), thr, t.T, tid, 256);
    for (int i = tid; i <= t.T; i += 256) cnt[i] = 0u;
    if (t.rank)
        for (int i = tid; i < t.T; i += 256) atl[i] = at_least[i];
    __syncthreads();
    t.tree = tree;
    t.cnt = cnt;
    t.at_least = atl;
    a.nbad = 0u;
    a.rank2 = 0ull;
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, l15, g);
    const int ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const unsigned nwg = gridDim.x;
    const unsigned wg = (nwg & 7u) == 0u ? (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int it0 = (int)(items * wg / nwg), it1 = (int)(items * (wg + 1) / nwg);
    if (mode == 2)
        ap_items<NI, 0, true, TK_CNT>(w, k, true, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, nullptr, nullptr, &a);
    else
        ap_items<NI, 0, false, TK_CNT>(w, k, mode != 0, R, M, Ab, Cb, ur, prow, pcol, nullptr, 0, it0, it1, nullptr, nullptr, &a);
    thr_close(t, tail, a.nbad, a.rank2, slabs + (size_t)blockIdx.x * slab_words(t.T), tid, 256);
}

static int eval_block_rows(const sgpr_handle* h, int R, int M) {
    const int64_t ncc = (M + AP_COLS - 1) / AP_COLS;
    const int64_t slots = (int64_t)h->num_cus * TK_OCC;
    int64_t rg = AB_ROWS / AP_ROWS;
    if (slots * EV_ITEMS_PER_WG / ncc < rg) rg = slots * EV_ITEMS_PER_WG / ncc;
    if (0x7fffffffLL / ncc < rg) rg = 0x7fffffffLL / ncc;
    rg = rg < 1 ? 1 : rg;
    return (int)(rg * AP_ROWS < R ? rg * AP_ROWS : R);
}

size_t score_eval_ws_bytes(const sgpr_handle* h, int R, int M, int T) {
    if (R == 0 || M == 0) return 0;
    const int rb = eval_block_rows(h, R, M);
    const size_t ncc = (size_t)(M + AP_COLS - 1) / AP_COLS;
    size_t b = a256(ncc * 4 * sizeof(double)) + a256(score_all_pairs_ws_bytes(rb, M));
    if (T >= 0) b += a256((size_t)topk_grid(h, rb, M) * slab_words(T) * sizeof(unsigned));
    return b + (rb < R ? 256 : 0);                        // (more than one block: the call's range, launch_call_range)
}

// the pose rule's squared class boundaries and the squared gaps that rule a work item out (EvalArgs, MineArgs)
template <class Args>
static void set_pose_cuts(Args& a, double d_pos, double d_neg) {
    a.lo2 = d_pos * d_pos;
    a.hi2 = d_neg * d_neg;
    a.cut_pos = a.lo2 * 1.001;
    a.cut_neg = (a.lo2 > a.hi2 ? a.lo2 : a.hi2) * 1.001;
}

int launch_score_eval(const sgpr_handle* h, const float* rows, int R, const float* cols, int M, const PairTruth& truth,
                      float* out, int64_t cap, unsigned long long* count, const float* thr, int T,
                      const sgpr_rank_group* rank, int gpt, const unsigned long long* at_least, unsigned long long* d_out,
                      void* ws, hipStream_t stream) {
    const bool counts = count == nullptr;
    hipError_t e = counts ? hipMemsetAsync(d_out, 0, (size_t)(T + 3) * sizeof(unsigned long long), stream)
                          : hipMemsetAsync(count, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return hip_fail(e, "fused evaluation: clearing the outputs");
    if ((int64_t)R * M == 0) return SGPR_OK;
    const int rb = eval_block_rows(h, R, M), ncc = (M + AP_COLS - 1) / AP_COLS;
    unsigned char* p = static_cast<unsigned char*>(ws);
    double* cbox = reinterpret_cast<double*>(p);
    p += a256((size_t)ncc * 4 * sizeof(double));
    unsigned* slabs = nullptr;
    const int sw = slab_words(T < 0 ? 0 : T);
    if (counts) {
        slabs = reinterpret_cast<unsigned*>(p);
        p += a256((size_t)topk_grid(h, rb, M) * sw * sizeof(unsigned));
    }
    if (truth.pose) {
        hipLaunchKernelGGL(eval_colbox_kernel, dim3((unsigned)ncc), dim3(64), 0, stream, truth.pose, M, cbox);
        if (int rc = launched("eval_colbox_kernel launch")) return rc;
    }
    EvalArgs a;
    memset(&a, 0, sizeof(a));
    a.truth = truth;
    set_pose_cuts(a, truth.d_pos, truth.d_neg);
    a.cbox = cbox;
    a.out = out;
    a.cap = cap;
    a.count = count;
    a.th.rank = rank;
    a.th.gpt = rank ? gpt : 0;
    a.th.T = T < 0 ? 0 : T;
    float* crng = nullptr;                                // more than one block: the f16 range of the whole rectangle
    if (rb < R) {
        crng = reinterpret_cast<float*>(p + a256(score_all_pairs_ws_bytes(rb, M)));
        const int rc = launch_call_range(h, rows, R, cols, M, rb, p, crng, stream);
        if (rc != SGPR_OK) return rc;
    }
    for (int r0 = 0; r0 < R; r0 += rb) {
        const int n = R - r0 < rb ? R - r0 : rb;
        const int nrng = 2 * ap_prep_groups(n, M);
        const ApOperands o = ap_operands(p, n, nrng, 2);
        const float* krng = crng ? crng : o.rng;
        const int knrng = crng ? 1 : nrng;
        const float* brows = rows + (size_t)r0 * F;
        a.truth.row0 = truth.row0 + r0;
        a.truth.gt = truth.gt ? truth.gt + (int64_t)r0 * truth.ldg : nullptr;
        const int rc = launch_ntn_prep(h, brows, n, cols, M, o, nrng, stream);
        if (rc != SGPR_OK) return rc;
        const int64_t grid = topk_grid(h, n, M);
        const dim3 gd((unsigned)grid), bd(256);
        if (!counts) {
            hipLaunchKernelGGL((score_positives_kernel<TK_OCC, AP_NI>), gd, bd, 0, stream, h->w, n, M, o.Ab, o.Cb, o.ur, krng,
                               knrng, brows, cols, a);
            if (int rc = launched("score_positives_kernel launch")) return rc;
            continue;
        }
        hipLaunchKernelGGL((score_counts_kernel<TK_OCC, AP_NI>), gd, bd, 0, stream, h->w, n, M, o.Ab, o.Cb, o.ur, krng, knrng,
                           brows, cols, a, thr, at_least, slabs);
        if (int rc = launched("score_counts_kernel launch")) return rc;
        const int rc2 = launch_slab_fold(slabs, (int)grid, sw, T, d_out, r0 > 0 ? 1 : 0, nullptr, 1, stream);
        if (rc2 != SGPR_OK) return rc2;
    }
    return SGPR_OK;
}

// ------------------------------------------------------------------ fused score + mining (sgpr_score_mine)
// workspace: sgpr_score_topk's | column boxes [ncc][4] f64 | row poses [R][2] f64 | row boxes [ceil(R / 4)][4] f64

// the pose of every row (d_row_pose[r], or the column pose of its own frame; NaN when that lies outside [0, M)) and the
// box of every four rows a wave of ap_items takes (ev_row_box's rule: a NaN pose widens the box to the plane)
__global__ __launch_bounds__(256) void mine_rowpose_kernel(int R, int M, const int32_t* __restrict__ row_self, int row0,
                                                           const double* __restrict__ row_pose,
                                                           const double* __restrict__ col_pose, double* __restrict__ rpose,
                                                           double* __restrict__ rbox) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q * 4 >= R) return;
    double bx[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int r = 4 * q; r < min(R, 4 * q + 4); ++r) {
        double px, pz;
        const long long s = row_self ? (long long)row_self[r] : (long long)row0 + r;
        if (row_pose) {
            px = row_pose[2 * (size_t)r];
            pz = row_pose[2 * (size_t)r + 1];
        } else if (s >= 0 && s < M) {
            px = col_pose[2 * (size_t)s];
            pz = col_pose[2 * (size_t)s + 1];
        } else {
            px = pz = __longlong_as_double(0x7ff8000000000000LL);
        }
        rpose[2 * (size_t)r] = px;
        rpose[2 * (size_t)r + 1] = pz;
        const bool nan = px != px || pz != pz;
        bx[0] = fmin(bx[0], nan ? -INFINITY : px);
        bx[1] = fmax(bx[1], nan ? INFINITY : px);
        bx[2] = fmin(bx[2], nan ? -INFINITY : pz);
        bx[3] = fmax(bx[3], nan ? INFINITY : pz);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) rbox[4 * (size_t)q + i] = bx[i];
}
__global__ __launch_bounds__(256) void mine_fill_kernel(int64_t n, float v, float* __restrict__ val,
                                                        int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        val[i] = v;
        idx[i] = -1;
    }
}

size_t score_mine_ws_bytes(const sgpr_handle* h, int R, int M, int k) {
    if (R == 0 || M == 0) return 0;
    return a256(score_topk_ws_bytes(h, R, M, k)) + a256((size_t)((M + AP_COLS - 1) / AP_COLS) * 4 * sizeof(double)) +
           a256((size_t)R * 2 * sizeof(double)) + (size_t)((R + 3) / 4) * 4 * sizeof(double);
}

int launch_score_mine(const sgpr_handle* h, const PooledRect& p, const Eligible& e, const MineSpec& mine,
                      const ListOut& out, void* ws, hipStream_t stream) {
    const int R = p.R, M = p.M, k = out.k, positives = mine.positives;
    const float *rows = p.rows, *cols = p.cols;
    const double *col_pose = mine.col_pose, d_pos = mine.d_pos, d_neg = mine.d_neg;
    if (R == 0) return SGPR_OK;
    if (M == 0) {                                          // no column at all: every slot is empty
        const int64_t n = (int64_t)R * k;
        hipLaunchKernelGGL(mine_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n,
                           positives ? INFINITY : -INFINITY, out.val, out.idx);
        return launched("mine_fill_kernel launch");
    }
    const int nrng = 2 * ap_prep_groups(R, M), ncc = (M + AP_COLS - 1) / AP_COLS;
    const ApOperands o = ap_operands(ws, R, nrng, 2);
    const int64_t items = (int64_t)ncc * ((R + AP_ROWS - 1) / AP_ROWS);
    const int64_t grid = std::min<int64_t>(items, (int64_t)h->num_cus * MN_OCC);   // (<= topk_grid: the lists fit)
    // (c != self_r: a window of at least 0 cuts the own frame out)
    Eligible cut = e;
    if (cut.window < 0) cut.window = 0;
    const TopkArgs a = topk_args(h, R, M, cut, out, ws);
    MineArgs m;
    memset(&m, 0, sizeof(m));
    m.truth.pose = col_pose;
    m.truth.d_pos = d_pos;
    m.truth.d_neg = d_neg;
    unsigned char* base = static_cast<unsigned char*>(ws);
    double* cbox = reinterpret_cast<double*>(base + a256(score_topk_ws_bytes(h, R, M, k)));
    double* rpose = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(cbox) + a256((size_t)ncc * 4 * sizeof(double)));
    double* rbox = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(rpose) + a256((size_t)R * 2 * sizeof(double)));
    m.cbox = cbox;
    m.rpose = rpose;
    m.rbox = rbox;
    set_pose_cuts(m, d_pos, d_neg);
    hipLaunchKernelGGL(eval_colbox_kernel, dim3((unsigned)ncc), dim3(64), 0, stream, col_pose, M, cbox);
    if (int rc = launched("eval_colbox_kernel launch")) return rc;
    hipLaunchKernelGGL(mine_rowpose_kernel, dim3((unsigned)(((R + 3) / 4 + 255) / 256)), dim3(256), 0, stream, R, M,
                       e.row_self, e.row0, mine.row_pose, col_pose, rpose, rbox);
    if (int rc = launched("mine_rowpose_kernel launch")) return rc;
    int rc = launch_ntn_prep(h, rows, R, cols, M, o, nrng, stream);
    if (rc != SGPR_OK) return rc;
    const dim3 gd((unsigned)grid), bd(256), gm((unsigned)((R + AP_ROWS - 1) / AP_ROWS));
    if (positives)
        rc = launch_list_k(k, "score_mine_kernel launch", [&](auto K) {
            hipLaunchKernelGGL((score_mine_kernel<MN_OCC, AP_NI, K, MN_POS>), gd, bd, 0, stream, h->w, R, M, o.Ab, o.Cb, o.ur,
                               o.rng, nrng, rows, cols, a, m);
        });
    else
        rc = launch_list_k(k, "score_mine_kernel launch", [&](auto K) {
            hipLaunchKernelGGL((score_mine_kernel<MN_OCC, AP_NI, K, MN_NEG>), gd, bd, 0, stream, h->w, R, M, o.Ab, o.Cb, o.ur,
                               o.rng, nrng, rows, cols, a, m);
        });
    if (rc != SGPR_OK) return rc;
    // (the lists of the negatives are top-k's: its merge instances; the positives' take the negating ones)
    return launch_list_k(k, "topk_merge_kernel launch", [&](auto K) {
        if (positives)
            hipLaunchKernelGGL((topk_merge_kernel<K, true>), gm, bd, 0, stream, R, M, (int)grid, a);
        else
            hipLaunchKernelGGL((topk_merge_kernel<K>), gm, bd, 0, stream, R, M, (int)grid, a);
    });
}

// ------------------------------------------------------------------ grouped pair list (sgpr_score_pair_list)
// The reference's own evaluation loop walks a pair LIST (eval_batch.py:30-36: ~15 listed pairs per row graph, 10^4-10^5
// pairs over 10^3 graphs).  The list arrives grouped by row graph (sgpr_pair_plan, host): work item = (row graph, up to 16
// of its listed columns).  ntn_prep hoists A'_r / u_r for the DISTINCT row graphs and the two-plane copies of the column
// graphs exactly as for the dense rectangle; a wave then takes FOUR items at a time through the all-pairs inner loop -
// layer 1 (3 MFMAs), split, layer 2 (2 MFMAs), head - with the columns gathered by index, and the lane-swap
// transpose-reduce that gives lane group g the four rows of one item in the dense kernel gives it item g here.  Every
// instruction and operand of a pair is the one score_all_pairs_kernel would use for that (row, column): the scores are
// bit-identical to the dense matrix's entries.  Against score_pairs_kernel (one wave per pair, the 64 KB NTN weight
// re-read per pair): ~430 VALU + 290 VMEM instructions per pair there, ~3 + 0.5 here.
// workspace:  ur [NR][T] f32 | rng [2 groups][4] f32 | Ab [NR][2][64][8] f16 | Cg [M][2][32] f16
static inline int pl_prep_groups(int NR, int M) { return ((NR > M ? NR : M) + 15) / 16; }

size_t score_pair_list_ws_bytes(int NR, int M) {
    return (size_t)NR * T * sizeof(float) + (size_t)2 * pl_prep_groups(NR, M) * 4 * sizeof(float) +
           (size_t)NR * 2 * 64 * 8 * sizeof(unsigned short) + (size_t)M * 2 * F * sizeof(unsigned short);
}

__global__ __launch_bounds__(256) void ntn_prep_list_kernel(const DevWeights w, const float* __restrict__ rows,
                                                            const int32_t* __restrict__ row_ids, int NR,
                                                            const float* __restrict__ cols, int M,
                                                            unsigned short* __restrict__ Ab, float* __restrict__ ur,
                                                            float* __restrict__ rng, unsigned short* __restrict__ Cg) {
    ntn_prep_body<true>(w, rows, NR, cols, M, Ab, ur, rng, Cg, (int)blockIdx.x, row_ids);
}

struct PairPlan {                 // device views into the plan buffer (sgpr.h, sgpr_pair_plan)
    const int32_t* row_ids;       // [NR]          distinct row graphs, ascending
    const int32_t* item_row;      // [NI]          compact row (index into row_ids) of every work item
    const int32_t* item_beg;      // [NI + 1]      first listed pair of the item in cols / pos (an item holds <= 16)
    const int32_t* cols;          // [P]           column graph of every listed pair, grouped by row graph
    const int32_t* pos;           // [P]           position of that pair in the caller's list = where its score goes
    int NR, NI;
};

template <bool CL>
__device__ __forceinline__ void pl_items(const DevWeights& w, const ApConsts& k, const bool fast, const PairPlan pl,
                                         const unsigned short* __restrict__ Ab, const unsigned short* __restrict__ Cg,
                                         const float* __restrict__ ur, const float* __restrict__ prow,
                                         const float* __restrict__ pcol, float* __restrict__ score) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const f16x8 w1hi = k.w1hi, w1lo = k.w1lo;
    const float4 b1v = k.b1v, side = k.side;
    const float nl2e = k.nl2e;
    const float nb2 = k.nb2;
    const int nquad = (pl.NI + 3) >> 2;
    const int wave0 = (int)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int)gridDim.x * 4;
    for (int q4 = wave0; q4 < nquad; q4 += nwaves) {
        if (!fast) {        // inputs outside the f16 range: exact fp32 arithmetic, one pair per wave step
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                const int item = 4 * q4 + i;
                if (item >= pl.NI) break;
                const int beg = pl.item_beg[item], end = pl.item_beg[item + 1];
                const float* e1 = prow + (size_t)pl.row_ids[pl.item_row[item]] * F;
#pragma unroll 1
                for (int p = beg; p < end; ++p) {
                    const float sc = slow_pair(w, e1, pcol + (size_t)pl.cols[p] * F);
                    if (lane == 0) score[pl.pos[p]] = sc;
                }
            }
            continue;
        }
        float zb[4];
        int my_beg = 0, my_cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int item = min(4 * q4 + i, pl.NI - 1);
            const int beg = pl.item_beg[item];
            const int cnt = (4 * q4 + i < pl.NI) ? pl.item_beg[item + 1] - beg : 0;
            if (i == g) {
                my_beg = beg;
                my_cnt = cnt;
            }
            const int r = pl.item_row[item];
            const int c = pl.cols[beg + min(l15, max(cnt, 1) - 1)];             // slots past the item's end repeat its last pair
            const unsigned short* ap = Ab + ((size_t)r * 2 * 64 + lane) * 8;      // A'_r[t = l15][8g .. 8g+7]
            const f16x8 ah = *reinterpret_cast<const f16x8*>(ap);
            const f16x8 al = *reinterpret_cast<const f16x8*>(ap + 64 * 8);
            const float4 u = *reinterpret_cast<const float4*>(ur + (size_t)r * T + 4 * g);
            const unsigned short* cp = Cg + (size_t)c * (2 * F) + 8 * g;          // e2_c[8g .. 8g+7], column = MFMA column l15
            const f16x8 bh = *reinterpret_cast<const f16x8*>(cp);
            const f16x8 bl = *reinterpret_cast<const f16x8*>(cp + F);
            f32x4 h = mfma_f16(al, bh, f32x4{u.x, u.y, u.z, u.w});
            h = mfma_f16(ah, bl, h);
            h = mfma_f16(ah, bh, h);
            const f16x8 hb = split_relu4<CL>(h);
            f32x4 q = mfma_f16(w1lo, hb, f32x4{b1v.x, b1v.y, b1v.z, b1v.w});
            q = mfma_f16(w1hi, hb, q);
            const float t0 = __builtin_amdgcn_fmed3f(q[0], 0.f, side.x), t1 = __builtin_amdgcn_fmed3f(q[1], 0.f, side.y);
            const float t2 = __builtin_amdgcn_fmed3f(q[2], 0.f, side.z), t3 = __builtin_amdgcn_fmed3f(q[3], 0.f, side.w);
            zb[i] = (t0 + t1) + (t2 + t3);
        }
        const float p02 = swap32_add(zb[0], zb[2]);
        const float p13 = swap32_add(zb[1], zb[3]);
        const float zsel = swap16_add(p02, p13);             // lane group g: item g of the quad, its pair l15
        const float sc = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(zsel, nl2e, nb2)));
        if (l15 < my_cnt) score[pl.pos[my_beg + l15]] = sc;
    }
}

__global__ __launch_bounds__(256) void score_pair_list_kernel(const DevWeights w, const PairPlan pl,
                                                              const unsigned short* __restrict__ Ab,
                                                              const unsigned short* __restrict__ Cg,
                                                              const float* __restrict__ ur,
                                                              const float* __restrict__ rng, int nrng,
                                                              const float* __restrict__ prow,
                                                              const float* __restrict__ pcol,
                                                              float* __restrict__ score, const int exact) {
    const int lane = threadIdx.x & 63;
    float am = 0.f, um = 0.f, em = 0.f, l1 = 0.f;
    ap_range(rng, nrng, am, um, em, l1);
    const int mode = exact ? 0 : ap_mode(am, um, em, l1);
    const ApConsts k = ap_consts(w, lane & 15, lane >> 4);
    if (mode == 2)
        pl_items<true>(w, k, true, pl, Ab, Cg, ur, prow, pcol, score);
    else
        pl_items<false>(w, k, mode != 0, pl, Ab, Cg, ur, prow, pcol, score);
}

int launch_score_pair_list(const sgpr_handle* h, const float* rows, const float* cols, int M, const int32_t* plan,
                           int NR, int NI, int64_t P, float* score, void* ws, hipStream_t stream, bool exact) {
    if (P == 0 || NI == 0) return SGPR_OK;
    PairPlan pl;
    pl.row_ids = plan;
    pl.item_row = pl.row_ids + NR;
    pl.item_beg = pl.item_row + NI;
    pl.cols = pl.item_beg + NI + 1;
    pl.pos = pl.cols + P;
    pl.NR = NR;
    pl.NI = NI;
    const int nrng = 2 * pl_prep_groups(NR, M);
    const ApOperands o = ap_operands(ws, NR, nrng, 2);
    hipLaunchKernelGGL(ntn_prep_list_kernel, dim3(nrng), dim3(256), 0, stream, h->w, rows, pl.row_ids, NR, cols, M, o.Ab, o.ur,
                       o.rng, o.Cb);
    if (int rc = launched("ntn_prep_list_kernel launch")) return rc;
    const int64_t wgs = ((int64_t)(NI + 3) / 4 + 3) / 4;          // one quad of items per wave, four waves per workgroup
    const int64_t slots = (int64_t)h->num_cus * 8;
    const unsigned grid = (unsigned)(wgs < slots ? wgs : slots);
    hipLaunchKernelGGL(score_pair_list_kernel, dim3(grid), dim3(256), 0, stream, h->w, pl, o.Ab, o.Cb, o.ur, o.rng, nrng, rows,
                       cols, score, exact ? 1 : 0);
    return launched("score_pair_list_kernel launch");
}

}  // namespace sgpr

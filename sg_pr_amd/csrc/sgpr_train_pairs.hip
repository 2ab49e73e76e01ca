// Training: the tail of the network (tensor network -> fully_connected_first -> scoring_layer -> weighted BCE,
// layers_batch.py:70-83 / sg_net.py:128-137) over EVERY ordered pair of G pooled vectors, forward and backward, without
// a [G^2, F, T] intermediate.
//
// For the ordered pair (i, j), e_i = rep[i], e_j = rep[j]:
//     z_t = relu(sum_{f,g} e_i[f] W[f,g,t] e_j[g] + sum_f V[t,f] e_i[f] + sum_g V[t,F+g] e_j[g] + b_t)
//     h = relu(fc1_w z + fc1_b),  s = sigmoid(fc2_w . h + fc2_b),  pred[i,j] = s
//     loss = sum w l / sum w over the pairs with cls[i,j] in {0, 1} (y = cls, w = w_neg / w_pos)
//
// One workgroup OWNS one graph o and streams the OTHER graphs x in tiles of `jb`.  A row owner (o = i, x = j) folds its
// vector into the bilinear form once, in LDS:
//     A_i[g,t] = sum_f e_i[f] W[f,g,t] + V[t,F+g],   c_i[t] = sum_f V[t,f] e_i[f] + b_t,   z_pre[j,t] = c_i[t] + sum_g A_i[g,t] e_j[g]
// The forward is one pass of row owners.  The backward is a pass of row owners, which recomputes z and h, and a pass
// of column owners.  With dz[i,j,t] the gradient at z_pre,
//     row owner i:    dA_i[g,t] = sum_j e_j[g] dz[i,j,t],  dc_i = sum_j dz[i,j],  d e_i = W : dA_i + V[:, :F]^T dc_i
//     column owner j: dB_j[f,t] = sum_i e_i[f] dz[i,j,t],  dd_j = sum_i dz[i,j],  d e_j = W^T : dB_j + V[:, F:]^T dd_j
// are local to the owner: the row pass yields the row half of d_rep, the column pass the column half, and no workgroup
// ever adds into another one's vector.  The column pass recomputes nothing: the row pass leaves, per pair, dlogit (f32)
// and the two ReLU masks (one bit per tensor neuron / bottleneck neuron, 64 bits each) in the workspace - 20 bytes a
// pair - so that both halves differentiate the SAME forward (a column-side recomputation rounds z_pre differently,
// and a neuron whose pre-activation sits at the rounding error of zero would get two different masks).  The row
// owners also give every parameter gradient: the head's (d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b) and dc_i as per-owner fp64
// partials in a slab, dA_i [G,F,T] as f32; the finish kernel walks the owners in order: dW[f,g,t] = sum_i e_i[f]
// dA_i[g,t], dV[t,f] = sum_i dc_i[t] e_i[f], dV[t,F+g] = sum_i dA_i[g,t], db = sum_i dc_i, the head's sums, d_rep = row
// half + column half.
//
// Plain fp32 FMAs for z, h and the logit (the widths are runtime values down to T = 5 and the stages of a tile are a
// few thousand FMAs between two barriers: nothing for a 16x16x4 tile to amortise); every sum over pairs is an fp64
// accumulator with one owner thread.  No atomics, every order fixed: same inputs, same bits.
//
// Launches: forward  pairs_kernel<false> (G workgroups) -> loss_kernel (1 wave)
//           backward pairs_kernel<true> (G row owners) -> cols_kernel (G column owners) -> finish_kernel
#include <math.h>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int TP_THREADS = 256;
constexpr size_t TP_LDS = 160 * 1024;   // the whole LDS of a CU (the widest shapes need it at jb = 4)

struct PairsShape {
    int G, F, T, H, jb;
};

__host__ __device__ inline size_t tp_align(size_t v) { return (v + 15) & ~(size_t)15; }

// fp64 words of a row owner's slab entry: dc [T] | d_fc1_w [H T] | d_fc1_b [H] | d_fc2_w [H] | d_fc2_b [1]
__host__ __device__ inline size_t tp_slab_words(int T, int H) { return (size_t)T + (size_t)H * T + 2 * (size_t)H + 1; }

// workspace: loss slab double2 [G] | dA f32 [G][F T] | slab f64 [G][words] | d_rep halves f64 [2][G][F] |
//            z masks u64 [G][G] | h masks u64 [G][G] | dlogit f32 [G][G]
struct PairsWorkspace {
    size_t loss, dA, slab, halves, zmask, hmask, dl, total;
};
__host__ __device__ inline PairsWorkspace tp_workspace(int G, int F, int T, int H) {
    PairsWorkspace w;
    w.loss = 0;
    w.dA = w.loss + tp_align((size_t)G * sizeof(double2));
    w.slab = w.dA + tp_align((size_t)G * F * T * sizeof(float));
    w.halves = w.slab + tp_align((size_t)G * tp_slab_words(T, H) * sizeof(double));
    w.zmask = w.halves + tp_align((size_t)2 * G * F * sizeof(double));
    w.hmask = w.zmask + tp_align((size_t)G * G * sizeof(unsigned long long));
    w.dl = w.hmask + tp_align((size_t)G * G * sizeof(unsigned long long));
    w.total = w.dl + tp_align((size_t)G * G * sizeof(float));
    return w;
}

// dynamic LDS of pairs_kernel (bytes); the fp64 accumulators come first (8-byte alignment)
__host__ __device__ inline size_t tp_lds_bytes(int F, int T, int H, int jb, bool bwd) {
    size_t d = bwd ? (size_t)F * T + tp_slab_words(T, H) : 2 * (size_t)jb;               // doubles
    size_t f = (size_t)F * T + T + F + (size_t)H * (T + 1) + 2 * (size_t)H               // A, c, e_o, fc1_w, fc1_b, fc2_w
               + (size_t)jb * (F + 1) + (size_t)jb * T + (size_t)jb * H;                 // e_x, z, h
    if (bwd) f += (size_t)jb + (size_t)jb * H + (size_t)jb * T;                          // dlogit, dh, dz
    return d * sizeof(double) + f * sizeof(float);
}

// dynamic LDS of cols_kernel: dB [F T] + dd [T] doubles, masks 2 [jb] u64; fc1_w, fc2_w, e_x, dlogit, dh, dz floats
__host__ __device__ inline size_t tp_cols_lds_bytes(int F, int T, int H, int jb) {
    return ((size_t)F * T + T + 2 * (size_t)jb) * 8 +
           ((size_t)H * (T + 1) + H + (size_t)jb * (F + 1) + jb + (size_t)jb * H + (size_t)jb * T) * sizeof(float);
}

__device__ inline double wave_sum_fixed(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// One row owner per workgroup.
template <bool BWD>
__global__ __launch_bounds__(TP_THREADS) void pairs_kernel(
    const float* __restrict__ rep, const float* __restrict__ W, const float* __restrict__ V, const float* __restrict__ b,
    const float* __restrict__ fc1_w, const float* __restrict__ fc1_b, const float* __restrict__ fc2_w,
    const float* __restrict__ fc2_b, const unsigned char* __restrict__ cls, float w_neg, float w_pos, PairsShape sh,
    float* __restrict__ pred,                  // forward: written; backward: read
    double2* __restrict__ loss_slab,           // forward
    const float* __restrict__ dloss, const float* __restrict__ wsum, float* __restrict__ dA_out,
    double* __restrict__ slab, double* __restrict__ halves, unsigned long long* __restrict__ zmask,
    unsigned long long* __restrict__ hmask, float* __restrict__ dl_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int G = sh.G, F = sh.F, T = sh.T, H = sh.H, jb = sh.jb, tid = threadIdx.x;
    const int o = blockIdx.x;
    const int FT = F * T, T1 = T + 1, F1 = F + 1;
    const int nslab = BWD ? (int)tp_slab_words(T, H) : 0;

    double* dAs = reinterpret_cast<double*>(smem);           // BWD: [F T]; forward: lsum [jb], wsum [jb]
    double* acc = dAs + (BWD ? FT : 0);                      // BWD: the slab entry (dc | d_fc1_w | d_fc1_b | d_fc2_w | d_fc2_b)
    float* As = reinterpret_cast<float*>(acc + (BWD ? nslab : 2 * jb));   // [F][T]
    float* cs = As + FT;                                     // [T]
    float* eo = cs + T;                                      // [F]
    float* w1 = eo + F;                                      // [H][T + 1]
    float* b1 = w1 + H * T1;                                 // [H]
    float* w2 = b1 + H;                                      // [H]
    float* es = w2 + H;                                      // [jb][F + 1]
    float* zs = es + jb * F1;                                // [jb][T]
    float* hs = zs + jb * T;                                 // [jb][H]
    float* dls = hs + jb * H;                                // BWD [jb]
    float* dhs = dls + jb;                                   // BWD [jb][H]
    float* dzs = dhs + jb * H;                               // BWD [jb][T]

    for (int f = tid; f < F; f += TP_THREADS) eo[f] = rep[(size_t)o * F + f];
    for (int e = tid; e < H * T; e += TP_THREADS) w1[(e / T) * T1 + e % T] = fc1_w[e];
    for (int h = tid; h < H; h += TP_THREADS) {
        b1[h] = fc1_b[h];
        w2[h] = fc2_w[h];
    }
    if (BWD) {
        for (int e = tid; e < FT + nslab; e += TP_THREADS) dAs[e] = 0.0;     // dAs and acc are contiguous
    }
    __syncthreads();
    for (int e = tid; e < FT; e += TP_THREADS) {             // e = x T + t
        const int x = e / T, t = e - x * T;
        float a = V[(size_t)t * 2 * F + F + x];
        for (int y = 0; y < F; ++y) a = fmaf(W[(size_t)y * FT + e], eo[y], a);
        As[e] = a;
    }
    for (int t = tid; t < T; t += TP_THREADS) {
        float a = b[t];
        for (int y = 0; y < F; ++y) a = fmaf(V[(size_t)t * 2 * F + y], eo[y], a);
        cs[t] = a;
    }
    const float b2 = fc2_b[0];
    float gs = 0.f;
    if (BWD) {
        const float ws = wsum[0];
        gs = ws > 0.f ? dloss[0] / ws : 0.f;
    }
    double my_l = 0.0, my_w = 0.0;                           // forward: thread jl's sums over its columns
    __syncthreads();

    for (int x0 = 0; x0 < G; x0 += jb) {
        const int nb = min(jb, G - x0);
        for (int e = tid; e < nb * F; e += TP_THREADS) {
            const int jl = e / F, g = e - jl * F;
            es[jl * F1 + g] = rep[(size_t)(x0 + jl) * F + g];
        }
        __syncthreads();
        for (int e = tid; e < nb * T; e += TP_THREADS) {
            const int jl = e / T, t = e - jl * T;
            const float* er = es + jl * F1;
            float a = cs[t];
            for (int g = 0; g < F; ++g) a = fmaf(As[g * T + t], er[g], a);
            zs[e] = relu_keep_nan(a);
        }
        __syncthreads();
        for (int e = tid; e < nb * H; e += TP_THREADS) {
            const int jl = e / H, h = e - jl * H;
            const float* zr = zs + jl * T;
            const float* wr = w1 + h * T1;
            float a = b1[h];
            for (int t = 0; t < T; ++t) a = fmaf(wr[t], zr[t], a);
            hs[e] = relu_keep_nan(a);
        }
        __syncthreads();
        if (tid < nb) {
            const int x = x0 + tid;
            const size_t pi = (size_t)o * G + x;             // (i, j) of this pair
            const unsigned char c = cls[pi];
            const float w = c == 0 ? w_neg : (c == 1 ? w_pos : 0.f);
            if (!BWD) {
                const float* hr = hs + tid * H;
                float a = b2;
                for (int h = 0; h < H; ++h) a = fmaf(w2[h], hr[h], a);
                const float s = 1.f / (1.f + expf(-a));
                pred[pi] = s;
                if (c <= 1) {
                    const double lg = c == 1 ? log((double)s) : log(1.0 - (double)s);   // -inf at s = 0 / 1
                    my_l += (double)w * -(lg < -100.0 ? -100.0 : lg);   // (torch's clamp: a NaN stays a NaN)
                    my_w += (double)w;
                }
            } else {
                float dl = 0.f;
                if (c <= 1) {
                    // torch's chain (s - y) / max(s (1 - s), 1e-12) * s (1 - s) on the fp32 s, so that a saturated s
                    // gives exactly 0; but s - 1 from the logit (the forward's bits again), not from the rounded s:
                    // near s = 1 one ulp of s is a large share of 1 - s
                    const float* hr = hs + tid * H;
                    float a = b2;
                    for (int h = 0; h < H; ++h) a = fmaf(w2[h], hr[h], a);
                    const float s = pred[pi], q = (1.f - s) * s;
                    const float d = c == 1 ? -1.f / (1.f + expf(a)) : s;
                    dl = (w * gs) * d / fmaxf(q, 1e-12f) * q;
                }
                dls[tid] = dl;
                dl_out[pi] = dl;
                if (dl != 0.f) {                             // the forward's ReLU masks, for the column pass
                    unsigned long long zm = 0ull, hm = 0ull;
                    // (!(v <= 0): v > 0 or NaN - torch's ReLU backward hands the gradient of a NaN activation on)
                    for (int t = 0; t < T; ++t) zm |= (unsigned long long)!(zs[tid * T + t] <= 0.f) << t;
                    for (int h = 0; h < H; ++h) hm |= (unsigned long long)!(hs[tid * H + h] <= 0.f) << h;
                    zmask[pi] = zm;
                    hmask[pi] = hm;
                }
            }
        }
        if (BWD) {
            __syncthreads();
            for (int e = tid; e < nb * H; e += TP_THREADS) {
                const int jl = e / H, h = e - jl * H;
                dhs[e] = !(hs[e] <= 0.f) ? dls[jl] * w2[h] : 0.f;
            }
            __syncthreads();
            for (int e = tid; e < nb * T; e += TP_THREADS) {
                const int jl = e / T, t = e - jl * T;
                float a = 0.f;
                if (!(zs[e] <= 0.f)) {
                    const float* dr = dhs + jl * H;
                    for (int h = 0; h < H; ++h) a = fmaf(w1[h * T1 + t], dr[h], a);
                }
                dzs[e] = a;
            }
            __syncthreads();
            for (int e = tid; e < FT; e += TP_THREADS) {     // dA[x,t] += sum over the tile of e_x[x] dz[t]
                const int g = e / T, t = e - g * T;
                double a = dAs[e];
                for (int jl = 0; jl < nb; ++jl) a += (double)es[jl * F1 + g] * (double)dzs[jl * T + t];
                dAs[e] = a;
            }
            for (int t = tid; t < T; t += TP_THREADS) {
                double a = acc[t];
                for (int jl = 0; jl < nb; ++jl) a += (double)dzs[jl * T + t];
                acc[t] = a;
            }
            {
                double* dW1 = acc + T;
                for (int e = tid; e < H * T; e += TP_THREADS) {
                    const int h = e / T, t = e - h * T;
                    double a = dW1[e];
                    for (int jl = 0; jl < nb; ++jl) a += (double)dhs[jl * H + h] * (double)zs[jl * T + t];
                    dW1[e] = a;
                }
                double* db1 = dW1 + H * T;
                double* dw2 = db1 + H;
                for (int h = tid; h < H; h += TP_THREADS) {
                    double a1 = db1[h], a2 = dw2[h];
                    for (int jl = 0; jl < nb; ++jl) {
                        a1 += (double)dhs[jl * H + h];
                        a2 += (double)dls[jl] * (double)hs[jl * H + h];
                    }
                    db1[h] = a1;
                    dw2[h] = a2;
                }
                if (tid == 0) {
                    double a = dw2[H];
                    for (int jl = 0; jl < nb; ++jl) a += (double)dls[jl];
                    dw2[H] = a;
                }
            }
        }
        __syncthreads();
    }

    if (!BWD) {
        if (tid < jb) {
            dAs[tid] = my_l;
            dAs[jb + tid] = my_w;
        }
        __syncthreads();
        if (tid == 0) {
            double l = 0.0, w = 0.0;
            for (int jl = 0; jl < jb; ++jl) {
                l += dAs[jl];
                w += dAs[jb + jl];
            }
            loss_slab[o] = make_double2(l, w);
        }
        return;
    }
    // the row half of d_rep: d e_i[f] = sum_{g,t} W[f,g,t] dA[g,t] + sum_t V[t,f] dc[t]; one wave per f, lanes over
    // (g, t), a fixed shuffle tree
    const int lane = tid & 63, wave = tid >> 6;
    for (int y = wave; y < F; y += TP_THREADS / 64) {
        double a = 0.0;
        for (int e = lane; e < FT; e += 64) a += (double)W[(size_t)y * FT + e] * dAs[e];
        for (int t = lane; t < T; t += 64) a += (double)V[(size_t)t * 2 * F + y] * acc[t];
        a = wave_sum_fixed(a);
        if (lane == 0) halves[(size_t)o * F + y] = a;
    }
    for (int e = tid; e < FT; e += TP_THREADS) dA_out[(size_t)o * FT + e] = (float)dAs[e];
    for (int e = tid; e < nslab; e += TP_THREADS) slab[(size_t)o * nslab + e] = acc[e];
}

// One column owner j per workgroup: the column half of d_rep from what the row pass left per pair (dlogit, ReLU masks).
__global__ __launch_bounds__(TP_THREADS) void cols_kernel(
    const float* __restrict__ rep, const float* __restrict__ W, const float* __restrict__ V,
    const float* __restrict__ fc1_w, const float* __restrict__ fc2_w, PairsShape sh,
    const unsigned long long* __restrict__ zmask, const unsigned long long* __restrict__ hmask,
    const float* __restrict__ dl_in, double* __restrict__ halves) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int G = sh.G, F = sh.F, T = sh.T, H = sh.H, jb = sh.jb, tid = threadIdx.x;
    const int o = blockIdx.x, FT = F * T, T1 = T + 1, F1 = F + 1;
    double* dBs = reinterpret_cast<double*>(smem);                                 // [F][T]
    double* dd = dBs + FT;                                                         // [T]
    unsigned long long* zms = reinterpret_cast<unsigned long long*>(dd + T);      // [jb]
    unsigned long long* hms = zms + jb;                                            // [jb]
    float* w1 = reinterpret_cast<float*>(hms + jb);                                // [H][T + 1]
    float* w2 = w1 + H * T1;                                                       // [H]
    float* es = w2 + H;                                                            // [jb][F + 1]
    float* dls = es + jb * F1;                                                     // [jb]
    float* dhs = dls + jb;                                                         // [jb][H]
    float* dzs = dhs + jb * H;                                                     // [jb][T]
    for (int e = tid; e < H * T; e += TP_THREADS) w1[(e / T) * T1 + e % T] = fc1_w[e];
    for (int h = tid; h < H; h += TP_THREADS) w2[h] = fc2_w[h];
    for (int e = tid; e < FT + T; e += TP_THREADS) dBs[e] = 0.0;                   // dBs and dd are contiguous
    __syncthreads();
    for (int x0 = 0; x0 < G; x0 += jb) {
        const int nb = min(jb, G - x0);
        for (int e = tid; e < nb * F; e += TP_THREADS) {
            const int jl = e / F, f = e - jl * F;
            es[jl * F1 + f] = rep[(size_t)(x0 + jl) * F + f];
        }
        if (tid < nb) {
            const size_t pi = (size_t)(x0 + tid) * G + o;                          // (i, j)
            const float dl = dl_in[pi];
            dls[tid] = dl;
            zms[tid] = dl != 0.f ? zmask[pi] : 0ull;
            hms[tid] = dl != 0.f ? hmask[pi] : 0ull;
        }
        __syncthreads();
        for (int e = tid; e < nb * H; e += TP_THREADS) {
            const int jl = e / H, h = e - jl * H;
            dhs[e] = (hms[jl] >> h) & 1ull ? dls[jl] * w2[h] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < nb * T; e += TP_THREADS) {
            const int jl = e / T, t = e - jl * T;
            float a = 0.f;
            if ((zms[jl] >> t) & 1ull) {
                const float* dr = dhs + jl * H;
                for (int h = 0; h < H; ++h) a = fmaf(w1[h * T1 + t], dr[h], a);
            }
            dzs[e] = a;
        }
        __syncthreads();
        for (int e = tid; e < FT; e += TP_THREADS) {
            const int f = e / T, t = e - f * T;
            double a = dBs[e];
            for (int jl = 0; jl < nb; ++jl) a += (double)es[jl * F1 + f] * (double)dzs[jl * T + t];
            dBs[e] = a;
        }
        for (int t = tid; t < T; t += TP_THREADS) {
            double a = dd[t];
            for (int jl = 0; jl < nb; ++jl) a += (double)dzs[jl * T + t];
            dd[t] = a;
        }
        __syncthreads();
    }
    // d e_j[g] = sum_{f,t} W[f,g,t] dB[f,t] + sum_t V[t,F+g] dd[t]
    const int lane = tid & 63, wave = tid >> 6;
    for (int y = wave; y < F; y += TP_THREADS / 64) {
        double a = 0.0;
        for (int e = lane; e < FT; e += 64) {
            const int x = e / T, t = e - x * T;
            a += (double)W[((size_t)x * F + y) * T + t] * dBs[e];
        }
        for (int t = lane; t < T; t += 64) a += (double)V[(size_t)t * 2 * F + F + y] * dd[t];
        a = wave_sum_fixed(a);
        if (lane == 0) halves[((size_t)G + o) * F + y] = a;
    }
}

__global__ __launch_bounds__(64) void loss_kernel(const double2* __restrict__ loss_slab, int G, float* __restrict__ loss,
                                                  float* __restrict__ wsum) {
    double l = 0.0, w = 0.0;
    for (int i = threadIdx.x; i < G; i += 64) {
        const double2 v = loss_slab[i];
        l += v.x;
        w += v.y;
    }
    l = wave_sum_fixed(l);
    w = wave_sum_fixed(w);
    if (threadIdx.x == 0) {
        loss[0] = w > 0.0 ? (float)(l / w) : 0.f;
        wsum[0] = (float)w;
    }
}

// One thread per output value, the owners walked in order.
// outputs: dW [F F T] | dV [T 2F] | db [T] | d_fc1_w [H T] | d_fc1_b [H] | d_fc2_w [H] | d_fc2_b [1] | d_rep [G F]
__global__ __launch_bounds__(TP_THREADS) void finish_kernel(const float* __restrict__ rep, const float* __restrict__ dA,
                                                            const double* __restrict__ slab,
                                                            const double* __restrict__ halves, PairsShape sh,
                                                            float* __restrict__ dW, float* __restrict__ dV,
                                                            float* __restrict__ db, float* __restrict__ d_fc1_w,
                                                            float* __restrict__ d_fc1_b, float* __restrict__ d_fc2_w,
                                                            float* __restrict__ d_fc2_b, float* __restrict__ d_rep) {
    const int G = sh.G, F = sh.F, T = sh.T, H = sh.H, FT = F * T;
    const long long nslab = (long long)tp_slab_words(T, H);
    const long long nW = (long long)F * FT, nV = 2LL * FT, nhead = nslab - T, nrep = (long long)G * F;
    long long e = (long long)blockIdx.x * TP_THREADS + threadIdx.x;
    if (e < nW) {
        const int f = (int)(e / FT), gt = (int)(e - (long long)f * FT);
        double a = 0.0;
        for (int i = 0; i < G; ++i) a += (double)rep[(size_t)i * F + f] * (double)dA[(size_t)i * FT + gt];
        dW[e] = (float)a;
        return;
    }
    e -= nW;
    if (e < nV) {
        const int t = (int)(e / (2 * F)), c = (int)(e - (long long)t * 2 * F);
        double a = 0.0;
        if (c < F) {
            for (int i = 0; i < G; ++i) a += slab[(size_t)i * nslab + t] * (double)rep[(size_t)i * F + c];
        } else {
            for (int i = 0; i < G; ++i) a += (double)dA[(size_t)i * FT + (size_t)(c - F) * T + t];
        }
        dV[e] = (float)a;
        return;
    }
    e -= nV;
    if (e < T + nhead) {                                     // db then the head, in the slab's own order
        double a = 0.0;
        for (int i = 0; i < G; ++i) a += slab[(size_t)i * nslab + e];
        float* out = e < T ? db + e
                           : (e < T + (long long)H * T ? d_fc1_w + (e - T)
                                                       : (e < T + (long long)H * T + H ? d_fc1_b + (e - T - (long long)H * T)
                                                                                       : (e < nslab - 1 ? d_fc2_w + (e - T - (long long)H * T - H)
                                                                                                        : d_fc2_b)));
        *out = (float)a;
        return;
    }
    e -= T + nhead;
    if (e < nrep) d_rep[e] = (float)(halves[e] + halves[nrep + e]);
}

static int tp_pick_tile(int F, int T, int H, bool bwd) {
    for (int jb = 16; jb >= 1; jb >>= 1)
        if (tp_lds_bytes(F, T, H, jb, bwd) <= TP_LDS) return jb;
    return 0;
}
static int tp_pick_cols_tile(int F, int T, int H) {
    for (int jb = 16; jb >= 1; jb >>= 1)
        if (tp_cols_lds_bytes(F, T, H, jb) <= TP_LDS) return jb;
    return 0;
}

static int tp_check(const char* what, int G, int F, int T, int H, const void* ws, size_t ws_bytes) {
    if (G < 1 || G > SGPR_TRAIN_PAIRS_MAX_GRAPHS || F < 1 || F > SGPR_ANY_MAX_FILTERS_3 || T < 1 ||
        T > SGPR_ANY_MAX_NEURONS || H < 1 || H > SGPR_ANY_MAX_NEURONS) {
        set_error(std::string(what) + ": G " + std::to_string(G) + ", F " + std::to_string(F) + ", T " + std::to_string(T) +
                  ", H " + std::to_string(H) + " outside 1 <= G <= " + std::to_string(SGPR_TRAIN_PAIRS_MAX_GRAPHS) +
                  ", 1 <= F <= " + std::to_string(SGPR_ANY_MAX_FILTERS_3) + ", 1 <= T, H <= " +
                  std::to_string(SGPR_ANY_MAX_NEURONS));
        return SGPR_E_DIMS;
    }
    if (!ws || ws_bytes < tp_workspace(G, F, T, H).total) {
        set_error(std::string(what) + ": workspace of " + std::to_string(tp_workspace(G, F, T, H).total) +
                  " bytes required (sgpr_pairs_train_workspace_bytes)");
        return SGPR_E_WORKSPACE;
    }
    return SGPR_OK;
}

static int tp_launched(const char* what) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, what);
}

}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_pairs_train_workspace_bytes(int G, int F, int T, int H) {
    if (G < 1 || G > SGPR_TRAIN_PAIRS_MAX_GRAPHS || F < 1 || F > SGPR_ANY_MAX_FILTERS_3 || T < 1 ||
        T > SGPR_ANY_MAX_NEURONS || H < 1 || H > SGPR_ANY_MAX_NEURONS)
        return 0;
    return tp_workspace(G, F, T, H).total;
}

int sgpr_pairs_train_forward(const float* d_rep, const float* d_W, const float* d_V, const float* d_b,
                             const float* d_fc1_w, const float* d_fc1_b, const float* d_fc2_w, const float* d_fc2_b,
                             const uint8_t* d_cls, float w_neg, float w_pos, int G, int F, int T, int H, float* d_pred,
                             float* d_loss, float* d_wsum, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* what = "sgpr_pairs_train_forward";
    if (!d_rep || !d_W || !d_V || !d_b || !d_fc1_w || !d_fc1_b || !d_fc2_w || !d_fc2_b || !d_cls || !d_pred || !d_loss ||
        !d_wsum) {
        set_error(std::string(what) + ": NULL argument");
        return SGPR_E_INVALID;
    }
    if (!(w_neg >= 0.f) || !(w_pos >= 0.f)) {
        set_error(std::string(what) + ": w_neg and w_pos must be >= 0");
        return SGPR_E_INVALID;
    }
    if (int rc = tp_check(what, G, F, T, H, d_workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PairsWorkspace w = tp_workspace(G, F, T, H);
    unsigned char* base = static_cast<unsigned char*>(d_workspace);
    double2* loss_slab = reinterpret_cast<double2*>(base + w.loss);
    PairsShape sh = {G, F, T, H, tp_pick_tile(F, T, H, false)};
    static LdsLimitOnce once;
    if (int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(&pairs_kernel<false>), (int)TP_LDS, what)) return rc;
    hipLaunchKernelGGL(pairs_kernel<false>, dim3(G), dim3(TP_THREADS), tp_lds_bytes(F, T, H, sh.jb, false), st, d_rep, d_W,
                       d_V, d_b, d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b, d_cls, w_neg, w_pos, sh, d_pred, loss_slab,
                       (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (double*)nullptr, (double*)nullptr,
                       (unsigned long long*)nullptr, (unsigned long long*)nullptr, (float*)nullptr);
    if (int rc = tp_launched("pairs_train forward pairs_kernel launch")) return rc;
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(64), 0, st, loss_slab, G, d_loss, d_wsum);
    return tp_launched("pairs_train loss_kernel launch");
}

int sgpr_pairs_train_backward(const float* d_dloss, const float* d_wsum, const float* d_pred, const float* d_rep,
                              const float* d_W, const float* d_V, const float* d_b, const float* d_fc1_w,
                              const float* d_fc1_b, const float* d_fc2_w, const float* d_fc2_b, const uint8_t* d_cls,
                              float w_neg, float w_pos, int G, int F, int T, int H, float* d_drep, float* d_dW,
                              float* d_dV, float* d_db, float* d_dfc1_w, float* d_dfc1_b, float* d_dfc2_w,
                              float* d_dfc2_b, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* what = "sgpr_pairs_train_backward";
    if (!d_dloss || !d_wsum || !d_pred || !d_rep || !d_W || !d_V || !d_b || !d_fc1_w || !d_fc1_b || !d_fc2_w ||
        !d_fc2_b || !d_cls || !d_drep || !d_dW || !d_dV || !d_db || !d_dfc1_w || !d_dfc1_b || !d_dfc2_w || !d_dfc2_b) {
        set_error(std::string(what) + ": NULL argument");
        return SGPR_E_INVALID;
    }
    if (!(w_neg >= 0.f) || !(w_pos >= 0.f)) {
        set_error(std::string(what) + ": w_neg and w_pos must be >= 0");
        return SGPR_E_INVALID;
    }
    if (int rc = tp_check(what, G, F, T, H, d_workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PairsWorkspace w = tp_workspace(G, F, T, H);
    unsigned char* base = static_cast<unsigned char*>(d_workspace);
    float* dA = reinterpret_cast<float*>(base + w.dA);
    double* slab = reinterpret_cast<double*>(base + w.slab);
    double* halves = reinterpret_cast<double*>(base + w.halves);
    PairsShape sh = {G, F, T, H, tp_pick_tile(F, T, H, true)};
    static LdsLimitOnce once;
    if (int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(&pairs_kernel<true>), (int)TP_LDS, what)) return rc;
    unsigned long long* zmask = reinterpret_cast<unsigned long long*>(base + w.zmask);
    unsigned long long* hmask = reinterpret_cast<unsigned long long*>(base + w.hmask);
    float* dl = reinterpret_cast<float*>(base + w.dl);
    hipLaunchKernelGGL(pairs_kernel<true>, dim3(G), dim3(TP_THREADS), tp_lds_bytes(F, T, H, sh.jb, true), st, d_rep,
                       d_W, d_V, d_b, d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b, d_cls, w_neg, w_pos, sh,
                       const_cast<float*>(d_pred), (double2*)nullptr, d_dloss, d_wsum, dA, slab, halves, zmask, hmask, dl);
    if (int rc = tp_launched("pairs_train backward pairs_kernel launch")) return rc;
    static LdsLimitOnce once_cols;
    if (int rc = raise_lds_limit(&once_cols, reinterpret_cast<const void*>(&cols_kernel), (int)TP_LDS, what)) return rc;
    PairsShape shc = {G, F, T, H, tp_pick_cols_tile(F, T, H)};
    hipLaunchKernelGGL(cols_kernel, dim3(G), dim3(TP_THREADS), tp_cols_lds_bytes(F, T, H, shc.jb), st, d_rep, d_W, d_V,
                       d_fc1_w, d_fc2_w, shc, zmask, hmask, dl, halves);
    if (int rc = tp_launched("pairs_train backward cols_kernel launch")) return rc;
    const long long outs = (long long)F * F * T + 2LL * F * T + (long long)tp_slab_words(T, H) + (long long)G * F;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((outs + TP_THREADS - 1) / TP_THREADS)), dim3(TP_THREADS), 0, st,
                       d_rep, dA, slab, halves, sh, d_dW, d_dV, d_db, d_dfc1_w, d_dfc1_b, d_dfc2_w, d_dfc2_b, d_drep);
    return tp_launched("pairs_train finish_kernel launch");
}

}  // extern "C"

// Training: one EdgeConv block of the reference (dgcnn.get_graph_feature -> Conv2d 1x1 -> BatchNorm2d with BATCH
// statistics -> LeakyReLU(0.2) -> max over the k neighbours, sg_net.py:50-73 / 79-110) forward and backward, without
// the [B, 2C, N, k] edge tensor.
//
// The 1x1 conv splits: with W = [Wa | Wb] over the channels (x_j - x_i, x_i),
//     z[b,f,i,k] = (Wa x)[b,f,j] + ((Wb - Wa) x)[b,f,i] = P[b,f,j] + Q[b,f,i],   j = idx[b,i,k]
// P and Q are per-node GEMMs the caller forms (hipBLASLt through torch, which also gives dW and dx).  Per channel, over
// all M = B N k edges (padded nodes included, as in the reference), the batch statistics follow from per-node sums of
// the gathered P: sum z = sum_i (S1_i + k Q_i), sum z^2 = sum_i (S2_i + 2 Q_i S1_i + k Q_i^2) with S1 = sum_k P_nbr,
// S2 = sum_k P_nbr^2.  BN + LeakyReLU is monotone in z (increasing for gamma >= 0, decreasing for gamma < 0), so the
// max over k needs the one edge with the largest (smallest) P; ties keep the lowest k.
//
// Backward, with g = dy * LReLU'(u_sel) on the selected edge and 0 on every other one:
//     dbeta = sum g,  dgamma = sum g xhat_sel,  xhat = (z - mean) / sigma
//     dQ_i = (gamma/sigma) (g_i - k dbeta/M - (dgamma/M) (S1_i + k Q_i - k mean) / sigma)
//     dP_j = (gamma/sigma) (G_j - indeg_j dbeta/M - (dgamma/M) (indeg_j (P_j - mean) + R_j) / sigma)
// G_j = sum of g over the selected edges that land on j, indeg_j = #(i,k) with idx = j, R_j = sum of Q_i over them.
//
// Launches (one workgroup per (graph, channel tile) unless noted):
//   forward : stats_kernel (P tile in LDS: gather, S1, S2, arg max / min; per-graph fp64 partial sums into a [B][F]
//             slab) -> reduce_kernel (one thread per channel sums the slab over b in order: mean, biased var)
//             -> apply_kernel (elementwise BN + LeakyReLU on the selected edge)
//   backward: grad_kernel (g, per-graph fp64 partials of dbeta / dgamma) -> reduce_kernel -> scatter_kernel (reverse
//             adjacency of the graph by a counting sort in LDS, each bucket put in edge order: dP by gathering over it,
//             dQ elementwise)
// No float atomics anywhere and every sum runs in a fixed order: results are bitwise reproducible.
#include <math.h>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int TR_THREADS = 256;
constexpr size_t TR_STAT_LDS = 56 * 1024;      // P tile budget of stats_kernel / grad_kernel (+ 4 KB of partials)
constexpr size_t TR_SCATTER_LDS = 160 * 1024;  // the whole LDS of a CU for scatter_kernel (the reverse list is N k words)

__host__ __device__ inline int row_pad(int N) { return N | 1; }   // odd row stride: channel-strided LDS reads spread

__device__ inline int clamp_node(long long j, int N) { return j < 0 ? 0 : (j >= N ? N - 1 : (int)j); }

__device__ inline float lrelu(float u) { return u > 0.f ? u : 0.2f * u; }

// fixed-order reduction of the TR_THREADS / FT partial pairs of each channel of the tile into the [B][F] slab
__device__ inline void tile_partials_to_slab(double a1, double a2, int FT, int nf, int b, int f0, int F, double2* slab) {
    __shared__ double r1[TR_THREADS], r2[TR_THREADS];
    const int tid = threadIdx.x;
    r1[tid] = a1;
    r2[tid] = a2;
    __syncthreads();
    if (tid < nf) {
        double s1 = 0.0, s2 = 0.0;
        for (int g = 0; g < TR_THREADS / FT; ++g) {
            s1 += r1[g * FT + tid];
            s2 += r2[g * FT + tid];
        }
        slab[(size_t)b * F + f0 + tid] = make_double2(s1, s2);
    }
}

// stage P[b, f0 : f0 + nf, :] into LDS rows of stride Np
__device__ inline void stage_tile(const float* __restrict__ src, float* dst, int b, int f0, int nf, int F, int N, int Np) {
    const float* s = src + ((size_t)b * F + f0) * N;
    for (int e = threadIdx.x; e < nf * N; e += TR_THREADS) dst[(e / N) * Np + e % N] = s[e];
}

// Forward pass 1.  Per (b, f, i): S1 (saved), the selected k (saved), z_sel = Q_i + P_sel into y (apply_kernel finishes
// it), and the graph's fp64 partials of sum z / sum z^2 per channel.
__global__ __launch_bounds__(TR_THREADS) void stats_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                           const long long* __restrict__ idx, const float* __restrict__ gamma,
                                                           int F, int N, int K, int FT, float* __restrict__ y,
                                                           unsigned char* __restrict__ sel, float* __restrict__ s1,
                                                           double2* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Ps = reinterpret_cast<float*>(smem);              // [FT][Np]
    const int b = blockIdx.x, f0 = blockIdx.y * FT, nf = min(FT, F - f0), Np = row_pad(N);
    stage_tile(P, Ps, b, f0, nf, F, N, Np);
    __syncthreads();
    const int tid = threadIdx.x, fl = tid % FT, ng = TR_THREADS / FT;
    double a1 = 0.0, a2 = 0.0;
    if (fl < nf) {
        const int f = f0 + fl;
        const bool neg = gamma[f] < 0.f;                       // gamma = 0 selects as gamma > 0
        const float* Pr = Ps + fl * Np;
        const long long* ib = idx + (size_t)b * N * K;
        const size_t row = ((size_t)b * F + f) * N;
        for (int i = tid / FT; i < N; i += ng) {
            double d1 = 0.0, d2 = 0.0;
            float best = 0.f;
            int bk = 0;
            for (int k = 0; k < K; ++k) {
                const float p = Pr[clamp_node(ib[(size_t)i * K + k], N)];
                d1 += (double)p;
                d2 += (double)p * (double)p;
                if (k == 0 || (neg ? p < best : p > best)) {   // strict: ties keep the lowest k
                    best = p;
                    bk = k;
                }
            }
            const float q = Q[row + i];
            const double qd = (double)q;
            a1 += d1 + (double)K * qd;
            a2 += d2 + 2.0 * qd * d1 + (double)K * qd * qd;
            s1[row + i] = (float)d1;
            sel[row + i] = (unsigned char)bk;
            y[row + i] = q + best;
        }
    }
    tile_partials_to_slab(a1, a2, FT, nf, b, f0, F, slab);
}

// mode 0: slab of (sum z, sum z^2) -> out0 = mean, out1 = biased variance;  mode 1: (sum g, sum g xhat) -> dbeta, dgamma
__global__ __launch_bounds__(TR_THREADS) void reduce_kernel(const double2* __restrict__ slab, int B, int F, double M,
                                                            int mode, float* __restrict__ out0, float* __restrict__ out1) {
    const int f = blockIdx.x * TR_THREADS + threadIdx.x;
    if (f >= F) return;
    double a = 0.0, c = 0.0;
    for (int b = 0; b < B; ++b) {
        const double2 v = slab[(size_t)b * F + f];
        a += v.x;
        c += v.y;
    }
    if (mode == 0) {
        const double mean = a / M;
        const double var = c / M - mean * mean;           // fp64: sums of up to 2^26 edges lose nothing that matters
        out0[f] = (float)mean;
        out1[f] = (float)(var > 0.0 ? var : 0.0);
    } else {
        out0[f] = (float)a;
        out1[f] = (float)c;
    }
}

__global__ __launch_bounds__(TR_THREADS) void apply_kernel(float* __restrict__ y, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean,
                                                           const float* __restrict__ var, float eps, int F, int N,
                                                           long long total) {
    const long long stride = (long long)gridDim.x * TR_THREADS;
    for (long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x; e < total; e += stride) {
        const int f = (int)((e / N) % F);
        const float xh = (y[e] - mean[f]) * (1.f / sqrtf(var[f] + eps));
        y[e] = lrelu(xh * gamma[f] + beta[f]);
    }
}

// Backward pass 1.  g = dy * LReLU'(u_sel) (into g_out = the caller's dQ buffer), fp64 partials of sum g / sum g xhat.
// z_sel is recomputed exactly as stats_kernel formed it (Q_i + P_sel in fp32).
__global__ __launch_bounds__(TR_THREADS) void grad_kernel(const float* __restrict__ dy, const float* __restrict__ P,
                                                          const float* __restrict__ Q, const long long* __restrict__ idx,
                                                          const unsigned char* __restrict__ sel,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, int F, int N, int K, int FT, float* __restrict__ g_out,
                                                          double2* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Ps = reinterpret_cast<float*>(smem);
    const int b = blockIdx.x, f0 = blockIdx.y * FT, nf = min(FT, F - f0), Np = row_pad(N);
    stage_tile(P, Ps, b, f0, nf, F, N, Np);
    __syncthreads();
    const int tid = threadIdx.x, fl = tid % FT, ng = TR_THREADS / FT;
    double a1 = 0.0, a2 = 0.0;
    if (fl < nf) {
        const int f = f0 + fl;
        const float mu = mean[f], inv = 1.f / sqrtf(var[f] + eps), ga = gamma[f], be = beta[f];
        const float* Pr = Ps + fl * Np;
        const long long* ib = idx + (size_t)b * N * K;
        const size_t row = ((size_t)b * F + f) * N;
        for (int i = tid / FT; i < N; i += ng) {
            const int k = min((int)sel[row + i], K - 1);
            const float z = Q[row + i] + Pr[clamp_node(ib[(size_t)i * K + k], N)];
            const float xh = (z - mu) * inv;
            const float g = xh * ga + be > 0.f ? dy[row + i] : 0.2f * dy[row + i];
            g_out[row + i] = g;
            a1 += (double)g;
            a2 += (double)g * (double)xh;
        }
    }
    tile_partials_to_slab(a1, a2, FT, nf, b, f0, F, slab);
}

// bytes of scatter_kernel's LDS ahead of the channel tiles: start[N + 1], cursor[N], scan[2][TR_THREADS], list[N k] u16
__host__ __device__ inline size_t scatter_fixed_bytes(int N, int K) {
    return ((size_t)(2 * N + 1 + 2 * TR_THREADS) * 4 + (size_t)N * K * 2 + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t scatter_tile_bytes(int N, int FT) {
    return (size_t)FT * (2 * (size_t)row_pad(N) * 4 + N);
}

// Backward pass 2.  The graph's edges are counting-sorted by target into LDS (integer counts; the placement order a
// bucket gets from the cursor atomics is then undone by sorting each bucket by edge id), so every dP_j sums its
// sources in edge order.  dQ is elementwise and overwrites the g that g_dq holds on entry.
__global__ __launch_bounds__(TR_THREADS) void scatter_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                             const long long* __restrict__ idx,
                                                             const unsigned char* __restrict__ sel,
                                                             const float* __restrict__ s1, const float* __restrict__ mean,
                                                             const float* __restrict__ var, const float* __restrict__ gamma,
                                                             const float* __restrict__ dbeta,
                                                             const float* __restrict__ dgamma, float eps, float M, int F,
                                                             int N, int K, int FT, float* __restrict__ dP,
                                                             float* __restrict__ g_dq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* start = reinterpret_cast<int*>(smem);                 // [N + 1]
    int* cur = start + N + 1;                                  // [N]: counts, then placement cursors
    int* scan = cur + N;                                       // [2][TR_THREADS]
    unsigned short* list = reinterpret_cast<unsigned short*>(scan + 2 * TR_THREADS);   // [N K] edge ids e = i K + k
    const int Np = row_pad(N);
    float* gs = reinterpret_cast<float*>(smem + scatter_fixed_bytes(N, K));   // [FT][Np]
    float* qs = gs + (size_t)FT * Np;                                         // [FT][Np]
    unsigned char* ss = reinterpret_cast<unsigned char*>(qs + (size_t)FT * Np);   // [FT][N]
    const int b = blockIdx.x, f0 = blockIdx.y * FT, nf = min(FT, F - f0), tid = threadIdx.x, NK = N * K;
    const long long* ib = idx + (size_t)b * NK;

    for (int j = tid; j < N; j += TR_THREADS) cur[j] = 0;
    stage_tile(g_dq, gs, b, f0, nf, F, N, Np);
    stage_tile(Q, qs, b, f0, nf, F, N, Np);
    {
        const unsigned char* s = sel + ((size_t)b * F + f0) * N;
        for (int e = tid; e < nf * N; e += TR_THREADS) ss[e] = s[e];
    }
    __syncthreads();
    for (int e = tid; e < NK; e += TR_THREADS) atomicAdd(&cur[clamp_node(ib[e], N)], 1);
    __syncthreads();
    // exclusive scan of the counts: per-thread chunks, a Hillis-Steele scan of the chunk sums
    const int chunk = (N + TR_THREADS - 1) / TR_THREADS, j0 = min(tid * chunk, N), j1 = min(j0 + chunk, N);
    int own = 0;
    for (int j = j0; j < j1; ++j) own += cur[j];
    scan[tid] = own;
    __syncthreads();
    int src = 0;
    for (int off = 1; off < TR_THREADS; off <<= 1) {
        const int v = scan[src * TR_THREADS + tid] + (tid >= off ? scan[src * TR_THREADS + tid - off] : 0);
        scan[(src ^ 1) * TR_THREADS + tid] = v;
        src ^= 1;
        __syncthreads();
    }
    int run = scan[src * TR_THREADS + tid] - own;
    for (int j = j0; j < j1; ++j) {
        const int c = cur[j];
        start[j] = run;
        cur[j] = run;
        run += c;
    }
    if (tid == 0) start[N] = NK;
    __syncthreads();
    for (int e = tid; e < NK; e += TR_THREADS) list[atomicAdd(&cur[clamp_node(ib[e], N)], 1)] = (unsigned short)e;
    __syncthreads();
    for (int j = tid; j < N; j += TR_THREADS) {                // buckets into edge order (insertion sort: ~k entries)
        const int lo = start[j], hi = start[j + 1];
        for (int p = lo + 1; p < hi; ++p) {
            const unsigned short v = list[p];
            int q = p;
            while (q > lo && list[q - 1] > v) {
                list[q] = list[q - 1];
                --q;
            }
            list[q] = v;
        }
    }
    __syncthreads();

    const int fl = tid % FT, ng = TR_THREADS / FT;
    if (fl >= nf) return;
    const int f = f0 + fl;
    const float mu = mean[f], inv = 1.f / sqrtf(var[f] + eps), c = gamma[f] * inv;
    const float db = dbeta[f] / M, dgs = dgamma[f] / M * inv;
    const float* gr = gs + fl * Np;
    const float* qr = qs + fl * Np;
    const unsigned char* sr = ss + fl * N;
    const size_t row = ((size_t)b * F + f) * N;
    for (int j = tid / FT; j < N; j += ng) {
        const int lo = start[j], hi = start[j + 1];
        float G = 0.f, R = 0.f;
        for (int p = lo; p < hi; ++p) {
            const int e = list[p], i = e / K, k = e - i * K;
            R += qr[i];
            if (sr[i] == k) G += gr[i];
        }
        const float deg = (float)(hi - lo);
        dP[row + j] = c * (G - deg * db - dgs * (deg * (P[row + j] - mu) + R));
        const float kf = (float)K;
        g_dq[row + j] = c * (gr[j] - kf * db - dgs * (s1[row + j] + kf * qr[j] - kf * mu));
    }
}

// largest power-of-two channel tile <= 64 (and <= F rounded up) whose LDS fits the budget; 0 if none
static int pick_tile(int F, int N, int K, bool scatter) {
    int ft = 1;
    while (ft < 64 && ft < F) ft <<= 1;
    for (; ft >= 1; ft >>= 1) {
        const size_t need = scatter ? scatter_fixed_bytes(N, K) + scatter_tile_bytes(N, ft)
                                    : (size_t)ft * row_pad(N) * sizeof(float);
        if (need <= (scatter ? TR_SCATTER_LDS : TR_STAT_LDS)) return ft;
    }
    return 0;
}

static size_t slab_bytes(int B, int F) { return (size_t)B * F * sizeof(double2); }

static int check_sizes(const char* what, int B, int F, int N, int K, float eps, size_t ws_bytes) {
    if (B < 1 || F < 1 || !(eps >= 0.f)) {
        set_error(std::string(what) + ": B and F must be >= 1 and eps >= 0");
        return SGPR_E_INVALID;
    }
    if (N < 1 || N > SGPR_TRAIN_MAX_NODES) {
        set_error(std::string(what) + ": N " + std::to_string(N) + " outside [1, " + std::to_string(SGPR_TRAIN_MAX_NODES) +
                  "]");
        return SGPR_E_NODES;
    }
    if (K < 1 || K > SGPR_TRAIN_MAX_K || K > N) {
        set_error(std::string(what) + ": K " + std::to_string(K) + " outside [1, min(N, " +
                  std::to_string(SGPR_TRAIN_MAX_K) + ")]");
        return SGPR_E_K;
    }
    // both launch shapes: stats / grad kernels on the 56 KB tile, scatter_kernel on the 160 KB one (either can be the
    // narrower); 64-bit, so that an F near INT_MAX cannot wrap the count
    const long long fs = pick_tile(F, N, K, false), fc = pick_tile(F, N, K, true);
    if ((F + fs - 1) / fs > 65535 || (F + fc - 1) / fc > 65535) {
        set_error(std::string(what) + ": F " + std::to_string(F) + " needs more channel tiles than one launch holds");
        return SGPR_E_DIMS;
    }
    if (ws_bytes < slab_bytes(B, F)) {
        set_error(std::string(what) + ": workspace of " + std::to_string(slab_bytes(B, F)) +
                  " bytes required (sgpr_edgeconv_train_workspace_bytes)");
        return SGPR_E_WORKSPACE;
    }
    return SGPR_OK;
}

static int reduce(const double2* slab, int B, int F, double M, int mode, float* o0, float* o1, hipStream_t st) {
    hipLaunchKernelGGL(reduce_kernel, dim3((F + TR_THREADS - 1) / TR_THREADS), dim3(TR_THREADS), 0, st, slab, B, F, M,
                       mode, o0, o1);
    return launched("edgeconv_train reduce_kernel launch");
}

}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_edgeconv_train_workspace_bytes(int B, int F) {
    return B > 0 && F > 0 ? slab_bytes(B, F) : 16;
}

int sgpr_edgeconv_train_forward(const float* d_P, const float* d_Q, const int64_t* d_idx, const float* d_gamma,
                                const float* d_beta, int B, int F, int N, int k, float eps, float* d_y,
                                uint8_t* d_sel, float* d_s1, float* d_mean, float* d_var, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    if (int rc = check_sizes("sgpr_edgeconv_train_forward", B, F, N, k, eps, workspace_bytes)) return rc;
    if (!d_P || !d_Q || !d_idx || !d_gamma || !d_beta || !d_y || !d_sel || !d_s1 || !d_mean || !d_var || !d_workspace) {
        set_error("sgpr_edgeconv_train_forward: NULL argument");
        return SGPR_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    double2* slab = static_cast<double2*>(d_workspace);
    const int ft = pick_tile(F, N, k, false);
    const long long* idx = reinterpret_cast<const long long*>(d_idx);
    hipLaunchKernelGGL(stats_kernel, dim3(B, (F + ft - 1) / ft), dim3(TR_THREADS),
                       (size_t)ft * row_pad(N) * sizeof(float), st, d_P, d_Q, idx, d_gamma, F, N, k, ft, d_y, d_sel,
                       d_s1, slab);
    if (int rc = launched("edgeconv_train stats_kernel launch")) return rc;
    if (int rc = reduce(slab, B, F, (double)B * N * k, 0, d_mean, d_var, st)) return rc;
    const long long total = (long long)B * F * N;
    long long blocks = (total + TR_THREADS - 1) / TR_THREADS;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)blocks), dim3(TR_THREADS), 0, st, d_y, d_gamma, d_beta, d_mean,
                       d_var, eps, F, N, total);
    return launched("edgeconv_train apply_kernel launch");
}

int sgpr_edgeconv_train_backward(const float* d_dy, const float* d_P, const float* d_Q, const int64_t* d_idx,
                                 const uint8_t* d_sel, const float* d_s1, const float* d_mean, const float* d_var,
                                 const float* d_gamma, const float* d_beta, int B, int F, int N, int k, float eps,
                                 float* d_dP, float* d_dQ, float* d_dgamma, float* d_dbeta, void* d_workspace,
                                 size_t workspace_bytes, void* stream) {
    if (int rc = check_sizes("sgpr_edgeconv_train_backward", B, F, N, k, eps, workspace_bytes)) return rc;
    if (!d_dy || !d_P || !d_Q || !d_idx || !d_sel || !d_s1 || !d_mean || !d_var || !d_gamma || !d_beta || !d_dP ||
        !d_dQ || !d_dgamma || !d_dbeta || !d_workspace) {
        set_error("sgpr_edgeconv_train_backward: NULL argument");
        return SGPR_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    double2* slab = static_cast<double2*>(d_workspace);
    const long long* idx = reinterpret_cast<const long long*>(d_idx);
    const int ft = pick_tile(F, N, k, false);
    hipLaunchKernelGGL(grad_kernel, dim3(B, (F + ft - 1) / ft), dim3(TR_THREADS),
                       (size_t)ft * row_pad(N) * sizeof(float), st, d_dy, d_P, d_Q, idx, d_sel, d_mean, d_var, d_gamma,
                       d_beta, eps, F, N, k, ft, d_dQ, slab);
    if (int rc = launched("edgeconv_train grad_kernel launch")) return rc;
    if (int rc = reduce(slab, B, F, 0.0, 1, d_dbeta, d_dgamma, st)) return rc;
    const int fs = pick_tile(F, N, k, true);
    const size_t lds = scatter_fixed_bytes(N, k) + scatter_tile_bytes(N, fs);
    static LdsLimitOnce once;
    if (int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(&scatter_kernel), (int)TR_SCATTER_LDS,
                                 "sgpr_edgeconv_train_backward"))
        return rc;
    hipLaunchKernelGGL(scatter_kernel, dim3(B, (F + fs - 1) / fs), dim3(TR_THREADS), lds, st, d_P, d_Q, idx, d_sel,
                       d_s1, d_mean, d_var, d_gamma, d_dbeta, d_dgamma, eps, (float)((double)B * N * k), F, N, k, fs,
                       d_dP, d_dQ);
    return launched("edgeconv_train scatter_kernel launch");
}

}  // extern "C"

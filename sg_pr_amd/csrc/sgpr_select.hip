// Large-k selection (sgpr_topk_rows_large, sgpr_score_topk_large): for every row of a resident n x M block (stride ld)
// the k <= SGPR_TOPK_LARGE_MAX best eligible columns, value descending then column ascending - the lists sgpr_topk_rows /
// sgpr_score_topk return for k <= 16.  DESIGN.md §15.
//
// Every entry becomes an order-preserving 32-bit key (-0 as +0; NaN, -inf and ineligible columns key 0, which never
// qualifies).  A row is cut into chunks of `chunk` columns, one workgroup per (chunk, row), so one long row spreads over
// the whole device and many short rows fill it as well:
//   sel_hist_kernel<p> / sel_pick_kernel<p>, p = 0, 1, 2: a radix select on digits of 11, 11 and 10 bits.  Each chunk
//       counts the keys that carry the prefix found so far into an LDS histogram and adds its non-zero bins to the row's
//       histogram (integer atomics: the sums do not depend on arrival order); one workgroup per row then finds the bin
//       that holds the k-th key and clears the histogram for the next pass.  After three passes the row knows the k-th
//       key T exactly and t, the number of entries equal to T that belong to the list (the others are above T).
//       A row with at most k qualifying entries takes them all (T = 0, t = 0) and skips the later passes.
//   sel_count_kernel: per chunk, the entries above T and those equal to T.
//   sel_scatter_kernel: an exclusive prefix over the chunks before it and a scan in column order inside the chunk place
//       the entries above T and the first t entries equal to T (lowest columns first: the tie rule) - (key, column)
//       parked in the caller's output row.
//   sel_sort_kernel: one workgroup per row sorts its survivors by (key descending, column ascending) in LDS (bitonic,
//       <= 4096 entries of 8 bytes), reads every value back from the block (the stored bits, -0.0 included) and pads
//       with (-inf, -1).
// Rows run in groups of at most SEL_GROUP, so the workspace is linear in min(n, SEL_GROUP) and in the chunk count.
#include <algorithm>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int SEL_THREADS = 256;
constexpr int SEL_TILE = 4 * SEL_THREADS;   // columns per workgroup step: four per thread (one 16-byte load)
constexpr int SEL_BINS = 2048;              // digits of 11, 11 and 10 bits
constexpr int SEL_GROUP = 4096;             // rows per round of launches

struct SelRows {
    const float* score;
    int M;
    int64_t ld;
    const int32_t* row_self;   // [n] or nullptr: self_r = row0 + r
    int row0, window, causal, k;
    int chunk, nch;            // columns per chunk (a multiple of SEL_TILE), chunks per row
    unsigned* hist;            // [rows][SEL_BINS]
    unsigned* state;           // [rows][4]: prefix / T, remaining k / t, entries taken, decided
    unsigned* cnt;             // [rows][nch][2]: above T, equal to T
    float* val;                // [rows][k]
    int32_t* idx;              // [rows][k]
    int32_t* status;
};

__device__ __forceinline__ int sel_self(const SelRows& a, int r) { return a.row_self ? a.row_self[r] : a.row0 + r; }

// columns at or past this one are never eligible (the causal rule); the window is tested per column
__device__ __forceinline__ int sel_lim(const SelRows& a, int self) {
    return a.causal ? (self < 0 ? 0 : (self < a.M ? self : a.M)) : a.M;
}

// the order-preserving image of a score: larger value, larger key; -0 and +0 one key; NaN and -inf key 0
__device__ __forceinline__ unsigned sel_key(float x) {
    if (!(x > -INFINITY)) return 0u;
    const unsigned u = __float_as_uint(x + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// keys of columns c .. c + 3 of row sp (0 at or past lim and inside the window); 16-byte loads when the row allows
__device__ __forceinline__ void sel_keys4(const SelRows& a, const float* sp, bool vec, int c, int lim, int self,
                                          unsigned (&key)[4]) {
    float x[4];
    if (vec && c + 3 < lim) {
        const float4 v = *reinterpret_cast<const float4*>(sp + c);
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = c + q < lim ? sp[c + q] : -INFINITY;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t dc = (int64_t)(c + q) - self;
        const bool ok = c + q < lim && (a.window < 0 || (dc < 0 ? -dc : dc) > a.window);
        key[q] = ok ? sel_key(x[q]) : 0u;
    }
}

// inclusive scan over the workgroup (four waves); total = the sum over all threads.  sh: 4 scratch words
template <class T>
__device__ __forceinline__ T sel_scan(T v, T* sh, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < SEL_THREADS / 64; ++i) {
        const T x = sh[i];
        base += i < w ? x : T(0);
        total += x;
    }
    __syncthreads();
    return v + base;
}

// one LDS count per entry: the bin of the first counting lane is added once for every lane that shares it (the scores
// crowd a few bins, and 64 lanes on one address would serialise), the other lanes add their own
__device__ __forceinline__ void sel_count(unsigned* h, bool in, unsigned bin) {
    const unsigned long long m = __ballot(in);
    if (!m) return;
    const int leader = __builtin_ctzll(m);
    const unsigned lb = __shfl(bin, leader);
    const unsigned long long same = __ballot(in && bin == lb);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lb], (unsigned)__popcll(same));
    else if (in && bin != lb) atomicAdd(&h[bin], 1u);
}

template <int PASS>
struct SelDigit {
    static constexpr int shift = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
    static constexpr int bins = PASS == 2 ? 1024 : 2048;
    static constexpr int above = PASS == 0 ? 32 : PASS == 1 ? 21 : 10;   // the prefix found so far: key bits above this
};

template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void sel_hist_kernel(SelRows a) {
    __shared__ unsigned h[SelDigit<PASS>::bins];
    const int r = blockIdx.y, tid = threadIdx.x;
    unsigned pre = 0;
    if (PASS > 0) {
        if (a.state[4 * r + 3]) return;                   // the row is decided
        pre = a.state[4 * r];
    }
    const int self = sel_self(a, r), lim = sel_lim(a, self);
    const int c0 = blockIdx.x * a.chunk, c1 = min(lim, c0 + a.chunk);
    if (c0 >= c1) return;
    for (int i = tid; i < SelDigit<PASS>::bins; i += SEL_THREADS) h[i] = 0;
    __syncthreads();
    const float* sp = a.score + (int64_t)r * a.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(sp) & 15) == 0;
    for (int t0 = c0; t0 < c1; t0 += SEL_TILE) {
        unsigned key[4];
        sel_keys4(a, sp, vec, t0 + 4 * tid, c1, self, key);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bool in = key[q] != 0u;
            if (PASS > 0) in = in && (key[q] >> SelDigit<PASS>::above) == (pre >> SelDigit<PASS>::above);
            sel_count(h, in, (key[q] >> SelDigit<PASS>::shift) & (SelDigit<PASS>::bins - 1));
        }
    }
    __syncthreads();
    unsigned* g = a.hist + (size_t)r * SEL_BINS;
    for (int i = tid; i < SelDigit<PASS>::bins; i += SEL_THREADS) {
        const unsigned v = h[i];
        if (v) atomicAdd(&g[i], v);
    }
}

// one workgroup per row: the bin holding the (remaining) k-th key, counted from the top; clears what it read
template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void sel_pick_kernel(SelRows a) {
    constexpr int NB = SelDigit<PASS>::bins, PER = NB / SEL_THREADS;
    __shared__ unsigned sh[SEL_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    unsigned* st = a.state + 4 * r;
    if (PASS == 0 && tid == 0 && a.row_self) {
        const int self = a.row_self[r];
        if (self < 0 || self >= a.M) atomicOr(a.status, 16);
    }
    if (PASS > 0 && st[3]) return;
    // (read by every thread before the scan's barriers; only the thread that finds the bin writes the state)
    const unsigned kp = PASS == 0 ? (unsigned)a.k : st[1], pre = PASS == 0 ? 0u : st[0];
    unsigned* g = a.hist + (size_t)r * SEL_BINS;
    unsigned c[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {                       // thread tid: bins NB-1-PER*tid downwards
        c[j] = g[NB - 1 - PER * tid - j];
        s += c[j];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) g[NB - 1 - PER * tid - j] = 0u;
    unsigned total;
    const unsigned incl = sel_scan(s, sh, total), excl = incl - s;
    if (PASS == 0 && total <= kp) {                       // at most k qualify: all of them, no boundary
        if (tid == 0) {
            st[0] = 0u;
            st[1] = 0u;
            st[2] = total;
            st[3] = 1u;
        }
        return;
    }
    if (excl < kp && kp <= incl) {                        // exactly one thread
        unsigned above = excl;
        int b = NB - 1 - PER * tid;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (above + c[j] >= kp) {
                b = NB - 1 - PER * tid - j;
                break;
            }
            above += c[j];
        }
        st[0] = pre | ((unsigned)b << SelDigit<PASS>::shift);
        st[1] = kp - above;
        st[2] = (unsigned)a.k;
        st[3] = PASS == 2 ? 1u : 0u;
    }
}

// per chunk: entries above T and entries equal to T (every chunk writes both, an empty one zeros)
__global__ __launch_bounds__(SEL_THREADS) void sel_count_kernel(SelRows a) {
    __shared__ unsigned long long sh[SEL_THREADS / 64];
    const int r = blockIdx.y, tid = threadIdx.x;
    const unsigned T = a.state[4 * r];
    const int self = sel_self(a, r), lim = sel_lim(a, self);
    const int c0 = blockIdx.x * a.chunk, c1 = min(lim, c0 + a.chunk);
    const float* sp = a.score + (int64_t)r * a.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(sp) & 15) == 0;
    unsigned gt = 0, eq = 0;
    for (int t0 = c0; t0 < c1; t0 += SEL_TILE) {
        unsigned key[4];
        sel_keys4(a, sp, vec, t0 + 4 * tid, c1, self, key);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            gt += key[q] > T ? 1u : 0u;
            eq += key[q] == T && T != 0u ? 1u : 0u;
        }
    }
    unsigned long long total;
    (void)sel_scan(((unsigned long long)gt << 32) | eq, sh, total);
    if (tid == 0) {
        unsigned* o = a.cnt + ((size_t)r * a.nch + blockIdx.x) * 2;
        o[0] = (unsigned)(total >> 32);
        o[1] = (unsigned)total;
    }
}

// the survivors of a chunk into slots of the row's output: above T at [prefix of the chunks before + rank], the first t
// equal to T (column order) at [g + rank], g = taken - t.  (key, column) parked as (bits, index) for sel_sort_kernel
__global__ __launch_bounds__(SEL_THREADS) void sel_scatter_kernel(SelRows a) {
    __shared__ unsigned long long sh[SEL_THREADS / 64];
    const int r = blockIdx.y, tid = threadIdx.x, ch = blockIdx.x;
    const unsigned T = a.state[4 * r], t = a.state[4 * r + 1], taken = a.state[4 * r + 2];
    const unsigned gtot = taken - t;
    unsigned long long part = 0, pre;
    for (int i = tid; i < ch; i += SEL_THREADS) {
        const unsigned* o = a.cnt + ((size_t)r * a.nch + i) * 2;
        part += ((unsigned long long)o[0] << 32) | o[1];
    }
    (void)sel_scan(part, sh, pre);                         // pre: the chunks before this one, summed
    const int self = sel_self(a, r), lim = sel_lim(a, self);
    const int c0 = ch * a.chunk, c1 = min(lim, c0 + a.chunk);
    if (c0 >= c1) return;
    const float* sp = a.score + (int64_t)r * a.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(sp) & 15) == 0;
    float* ov = a.val + (size_t)r * a.k;
    int32_t* oi = a.idx + (size_t)r * a.k;
    unsigned base_gt = (unsigned)(pre >> 32), base_eq = (unsigned)pre;
    for (int t0 = c0; t0 < c1; t0 += SEL_TILE) {
        const int c = t0 + 4 * tid;
        unsigned key[4], ngt = 0, neq = 0;
        sel_keys4(a, sp, vec, c, c1, self, key);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ngt += key[q] > T ? 1u : 0u;
            neq += key[q] == T && T != 0u ? 1u : 0u;
        }
        const unsigned long long mine = ((unsigned long long)ngt << 32) | neq;
        unsigned long long tot;
        const unsigned long long ex = sel_scan(mine, sh, tot) - mine;
        unsigned jg = base_gt + (unsigned)(ex >> 32), je = base_eq + (unsigned)ex;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned slot = 0xffffffffu;
            if (key[q] > T) {
                slot = jg++;
            } else if (key[q] == T && T != 0u) {
                if (je < t) slot = gtot + je;
                ++je;
            }
            if (slot < taken && slot < (unsigned)a.k) {
                reinterpret_cast<unsigned*>(ov)[slot] = key[q];
                oi[slot] = c + q;
            }
        }
        base_gt += (unsigned)(tot >> 32);
        base_eq += (unsigned)tot;
    }
}

// one workgroup per row: survivors sorted by (key descending, column ascending) in LDS, values read back from the block
__global__ __launch_bounds__(SEL_THREADS) void sel_sort_kernel(SelRows a, int P) {
    extern __shared__ unsigned long long sk[];
    const int r = blockIdx.x, tid = threadIdx.x;
    const unsigned taken = a.state[4 * r + 2];
    float* ov = a.val + (size_t)r * a.k;
    int32_t* oi = a.idx + (size_t)r * a.k;
    for (int i = tid; i < P; i += SEL_THREADS) {
        unsigned long long v = 0;
        if ((unsigned)i < taken && i < a.k)
            v = ((unsigned long long)reinterpret_cast<const unsigned*>(ov)[i] << 32) | (0xffffffffu - (unsigned)oi[i]);
        sk[i] = v;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += SEL_THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long x = sk[lo], y = sk[hi];
                if (desc ? x < y : x > y) {
                    sk[lo] = y;
                    sk[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    const float* sp = a.score + (int64_t)r * a.ld;
    for (int i = tid; i < a.k; i += SEL_THREADS) {
        const unsigned long long v = i < P ? sk[i] : 0ull;
        const unsigned col = 0xffffffffu - (unsigned)v;
        if ((v >> 32) && col < (unsigned)a.M) {
            ov[i] = sp[col];
            oi[i] = (int32_t)col;
        } else {
            ov[i] = -INFINITY;
            oi[i] = -1;
        }
    }
}

// M == 0: every slot padded; a row_self entry is out of range by definition
__global__ __launch_bounds__(SEL_THREADS) void sel_fill_kernel(int n, int k, const int32_t* row_self, float* val,
                                                               int32_t* idx, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (i < (int64_t)n * k) {
        val[i] = -INFINITY;
        idx[i] = -1;
    }
    if (row_self && i < n) atomicOr(status, 16);
}

// wide chunks while the grid has enough of them; a few long rows take narrow ones to reach every CU
static int sel_chunk(int n, int M) {
    const int64_t wide = (int64_t)n * ((M + 4 * SEL_TILE - 1) / (4 * SEL_TILE));
    return wide >= 1024 ? 4 * SEL_TILE : SEL_TILE;
}

// hist [G][SEL_BINS] | state [G][4] | chunk counts [G][M / SEL_TILE][2] (the narrowest chunk: any n up to this one fits)
size_t select_ws_bytes(int n, int M) {
    if (n <= 0 || M <= 0) return 0;
    const size_t g = (size_t)std::min(n, SEL_GROUP), nch = (size_t)((M + SEL_TILE - 1) / SEL_TILE);
    return a256(g * SEL_BINS * 4) + a256(g * 16) + a256(g * nch * 8);
}

// rows per round of launches for a block of n rows: what the workspace's layout depends on (the histograms of
// select_group_rows(n) rows come first, state and chunk counts behind them)
int select_group_rows(int n) { return std::min(n, SEL_GROUP); }

int launch_select_rows(const ScoreBlock& b, const Eligible& el, const ListOut& out, void* ws, bool ws_clean,
                       int32_t* status, hipStream_t s) {
    const int n = b.R, M = b.M, k = out.k;
    if (n == 0) return SGPR_OK;
    if (M == 0) {
        const int64_t total = std::max<int64_t>((int64_t)n * k, n);
        hipLaunchKernelGGL(sel_fill_kernel, dim3((unsigned)((total + SEL_THREADS - 1) / SEL_THREADS)), dim3(SEL_THREADS),
                           0, s, n, k, el.row_self, out.val, out.idx, status);
        return launched("sel_fill_kernel launch");
    }
    const int G = std::min(n, SEL_GROUP), chunk = sel_chunk(n, M), nch = (M + chunk - 1) / chunk;
    unsigned char* p = static_cast<unsigned char*>(ws);
    SelRows a;
    a.M = M;
    a.ld = b.ld;
    a.window = el.window;
    a.causal = el.causal;
    a.k = k;
    a.chunk = chunk;
    a.nch = nch;
    a.hist = reinterpret_cast<unsigned*>(p);
    a.state = reinterpret_cast<unsigned*>(p + a256((size_t)G * SEL_BINS * 4));
    a.cnt = reinterpret_cast<unsigned*>(p + a256((size_t)G * SEL_BINS * 4) + a256((size_t)G * 16));
    a.status = status;
    if (!ws_clean) {                                      // every pick clears what it read: one clear per call
        const hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)G * SEL_BINS * 4, s);
        if (e != hipSuccess) return hip_fail(e, "large top-k: clearing the histograms");
    }
    int P = 1;
    while (P < k) P <<= 1;
    const dim3 blk(SEL_THREADS);
    for (int r0 = 0; r0 < n; r0 += G) {
        const int g = std::min(G, n - r0);
        const Eligible eg = el.from(r0);
        const ListOut og = out.at(r0);
        a.score = b.score + (int64_t)r0 * b.ld;
        a.row_self = eg.row_self;
        a.row0 = eg.row0;
        a.val = og.val;
        a.idx = og.idx;
        const dim3 grid2((unsigned)nch, (unsigned)g), grid1((unsigned)g);
        hipLaunchKernelGGL(sel_hist_kernel<0>, grid2, blk, 0, s, a);
        hipLaunchKernelGGL(sel_pick_kernel<0>, grid1, blk, 0, s, a);
        hipLaunchKernelGGL(sel_hist_kernel<1>, grid2, blk, 0, s, a);
        hipLaunchKernelGGL(sel_pick_kernel<1>, grid1, blk, 0, s, a);
        hipLaunchKernelGGL(sel_hist_kernel<2>, grid2, blk, 0, s, a);
        hipLaunchKernelGGL(sel_pick_kernel<2>, grid1, blk, 0, s, a);
        hipLaunchKernelGGL(sel_count_kernel, grid2, blk, 0, s, a);
        hipLaunchKernelGGL(sel_scatter_kernel, grid2, blk, 0, s, a);
        hipLaunchKernelGGL(sel_sort_kernel, grid1, blk, (size_t)P * 8, s, a, P);
        const int rc = launched("large top-k launches");
        if (rc != SGPR_OK) return rc;
    }
    return SGPR_OK;
}

}  // namespace sgpr

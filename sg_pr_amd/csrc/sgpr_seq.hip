// Sequence matching (sgpr_seq_filter, sgpr_score_seq_topk; sgpr_seq_rows_above, sgpr_score_seq_above): the mean of the
// scores along the last L scans of both trajectories, i.e. along a diagonal of the similarity matrix that ends in (r, c).
// DESIGN.md §17, §18.
//
//   D(r, c)  = { d in 0..L-1 : r - d >= 0 and 0 <= c - sigma d < M }        sigma = +1 forward, -1 reverse
//   Q[r, c]  = (S[r, c] + S[r-1, c-sigma] + ...) * rcp[|D|]                 fp32 additions in ascending d
//
// Both conditions are monotone in d, so D is the prefix 0..n-1 with n = min(L, r + 1, c + 1) (forward) or
// min(L, r + 1, M - c) (reverse): each lane runs its own trip count and no term is ever masked or replaced by a zero
// (a zero would turn a -0.0 sum into +0.0).
//
// seq_filter_kernel: one workgroup per tile of SEQ_TR output rows x SEQ_TC columns.  It stages the
// (rows + L-1) x (SEQ_TC + 2 (L-1)) scores the tile's diagonals reach into LDS - lanes along a row, so every global load
// is a contiguous run, zero outside the rectangle - and then each thread owns one column and walks the tile's rows.  At
// step d lane i reads word (row - d) * pitch + i -+ d: adjacent lanes, adjacent words, in either direction (no bank
// conflict).  L is a runtime value; the LDS is sized by it at launch (80 136 bytes at L = 32).
#include <algorithm>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int SEQ_TR = 32;     // output rows per tile
constexpr int SEQ_TC = 256;    // columns per tile = threads per workgroup

struct SeqArgs {
    const float* score;   // [R][ld]
    int R, M;
    int64_t ld;
    int ctx, L, fwd, rev;
    float* out;           // [R - ctx][ldo]
    int64_t ldo;
    unsigned char* dir;   // [R - ctx][ldd] or nullptr
    int64_t ldd;
    int tiles_x;
    float rcp[SGPR_SEQ_MAX_LEN + 1];   // rcp[n] = (float)(1.0 / n), rounded once from double on the host
};

__global__ __launch_bounds__(SEQ_TC) void seq_filter_kernel(const SeqArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float seq_tile[];
    const int tid = threadIdx.x, h = a.L - 1;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int r_base = a.ctx + ty * SEQ_TR, c_base = tx * SEQ_TC;
    const int rows = min(SEQ_TR, a.R - r_base);          // output rows of this tile (>= 1 by the grid)
    const int pitch = SEQ_TC + 2 * h;
    // LDS row lr holds input row r_base - h + lr, LDS column lc input column c_base - h + lc
    for (int lr = 0; lr < rows + h; ++lr) {
        const int r = r_base - h + lr;                   // < R by construction
        const float* sp = a.score + (int64_t)(r < 0 ? 0 : r) * a.ld;
        for (int lc = tid; lc < pitch; lc += SEQ_TC) {
            const int c = c_base - h + lc;
            seq_tile[lr * pitch + lc] = (r >= 0 && c >= 0 && c < a.M) ? sp[c] : 0.f;
        }
    }
    __syncthreads();
    const int c = c_base + tid;
    if (c >= a.M) return;
    const int nc_f = min(a.L, c + 1), nc_r = min(a.L, a.M - c);
    for (int i = 0; i < rows; ++i) {
        const int r = r_base + i;
        const float* t0 = seq_tile + (i + h) * pitch + h + tid;
        const int nr = min(a.L, r + 1);
        const float s0 = t0[0];
        float qf = 0.f, qr = 0.f;
        if (a.fwd) {
            const int n = min(nr, nc_f);
            float s = s0;
            for (int d = 1; d < n; ++d) s = s + t0[-d * pitch - d];
            qf = s * a.rcp[n];
        }
        if (a.rev) {
            const int n = min(nr, nc_r);
            float s = s0;
            for (int d = 1; d < n; ++d) s = s + t0[-d * pitch + d];
            qr = s * a.rcp[n];
        }
        // both directions: reverse where it is larger or forward is NaN; forward wins ties
        const bool take_rev = a.rev && (!a.fwd || qr > qf || qf != qf);
        const int64_t o = (int64_t)(r - a.ctx);
        a.out[o * a.ldo + c] = take_rev ? qr : qf;
        if (a.dir) a.dir[o * a.ldd + c] = take_rev ? 1 : 0;
    }
}

int launch_seq_filter(const float* score, int R, int M, int64_t ld, int ctx, int L, int flags, float* out, int64_t ldo,
                      unsigned char* dir, int64_t ldd, hipStream_t s) {
    if (R - ctx <= 0 || M <= 0) return SGPR_OK;
    static LdsLimitOnce once;
    const int lds_max = (SEQ_TR + SGPR_SEQ_MAX_LEN - 1) * (SEQ_TC + 2 * (SGPR_SEQ_MAX_LEN - 1)) * (int)sizeof(float);
    int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(seq_filter_kernel), lds_max, "sequence filter");
    if (rc != SGPR_OK) return rc;
    SeqArgs a;
    a.score = score;
    a.R = R;
    a.M = M;
    a.ld = ld;
    a.ctx = ctx;
    a.L = L;
    a.fwd = (flags & SGPR_SEQ_FORWARD) ? 1 : 0;
    a.rev = (flags & SGPR_SEQ_REVERSE) ? 1 : 0;
    a.out = out;
    a.ldo = ldo;
    a.dir = dir;
    a.ldd = ldd;
    a.rcp[0] = 0.f;
    for (int n = 1; n <= SGPR_SEQ_MAX_LEN; ++n) a.rcp[n] = (float)(1.0 / n);
    const int64_t tx = (M + SEQ_TC - 1) / SEQ_TC, ty = (R - ctx + SEQ_TR - 1) / SEQ_TR;
    if (tx * ty > 0x7fffffffLL) {
        set_error("sequence filter: more than 2^31 tiles");
        return SGPR_E_INVALID;
    }
    a.tiles_x = (int)tx;
    const int rows = std::min(SEQ_TR, R - ctx);
    const size_t lds = (size_t)(rows + L - 1) * (SEQ_TC + 2 * (L - 1)) * sizeof(float);
    hipLaunchKernelGGL(seq_filter_kernel, dim3((unsigned)(tx * ty)), dim3(SEQ_TC), lds, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "seq_filter_kernel launch");
}

// ------------------------------------------------------------------ range selection on Q (sgpr_seq_rows_above, sgpr_score_seq_above)
// seq_above_kernel<PASS>: seq_filter_kernel's tile, staging and diagonal walks with a range-select epilogue in place of
// the stores of Q and dir.  A thread owns a column, a wave a 64-column segment of the tile.
//   pass 1    per output row: hit = eligible && q >= thr, one ballot; lane 0 stores its popcount to seg[o][segment].
//             Exactly one wave writes every (o, segment) entry, zeros included: no memset, nothing read from before.
//   row scan  seq_above_rowscan_kernel, one wave per output row: seg[o][*] -> exclusive offsets in place, cnt[o].
//   scan      above_scan_kernel (sgpr_score.hip): cnt -> row_ptr and the running total, continuing across row blocks.
//   pass 2    recomputes q (the same instructions): position = row_ptr[o] + seg[o][segment] + hits in the lanes below.
// Plain vector stores; the only atomic is the status OR of a row_self entry outside [0, M) (rows_above_kernel's bit).
struct SeqAboveArgs {
    const float* score;   // [R][ld]
    int R, M;
    int64_t ld;
    int ctx, L, fwd, rev;
    int tiles_x, nseg;    // nseg = ceil(M / 64)
    const int32_t* row_self;   // [R] or nullptr: row0 + r
    int row0, window, causal;
    float thr;
    int32_t* seg;         // [R - ctx][nseg]: pass 1 counts, then (row scan) the segment's offset within its row
    const int64_t* row_ptr;    // [R - ctx + 1] (pass 2)
    int rout0;            // output row of the first row after the context
    int32_t* rows;
    int32_t* cols;
    float* vals;
    unsigned char* dirs;  // or nullptr
    int64_t cap;
    int32_t* status;
    float rcp[SGPR_SEQ_MAX_LEN + 1];
};

template <int PASS>
__global__ __launch_bounds__(SEQ_TC) void seq_above_kernel(const SeqAboveArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float seq_tile[];
    const int tid = threadIdx.x, h = a.L - 1;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int r_base = a.ctx + ty * SEQ_TR, c_base = tx * SEQ_TC;
    const int rows = min(SEQ_TR, a.R - r_base);          // output rows of this tile (>= 1 by the grid)
    const int pitch = SEQ_TC + 2 * h;
    // LDS row lr holds input row r_base - h + lr, LDS column lc input column c_base - h + lc
    for (int lr = 0; lr < rows + h; ++lr) {
        const int r = r_base - h + lr;                   // < R by construction
        const float* sp = a.score + (int64_t)(r < 0 ? 0 : r) * a.ld;
        for (int lc = tid; lc < pitch; lc += SEQ_TC) {
            const int c = c_base - h + lc;
            seq_tile[lr * pitch + lc] = (r >= 0 && c >= 0 && c < a.M) ? sp[c] : 0.f;
        }
    }
    __syncthreads();
    const int lane = tid & 63, segment = tx * (SEQ_TC / 64) + (tid >> 6);
    if (segment >= a.nseg) return;                       // (a whole wave beyond M: no segment of its own, no barrier ahead)
    const int c = c_base + tid;
    // a tail lane of the wave that holds column M - 1 stays for the ballots, never a hit; its sums read staged zeros
    const bool in = c < a.M;
    const int nc_f = in ? min(a.L, c + 1) : 1, nc_r = in ? min(a.L, a.M - c) : 1;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = 0; i < rows; ++i) {
        const int r = r_base + i;
        const float* t0 = seq_tile + (i + h) * pitch + h + tid;
        const int nr = min(a.L, r + 1);
        const float s0 = t0[0];
        float qf = 0.f, qr = 0.f;
        if (a.fwd) {
            const int n = min(nr, nc_f);
            float s = s0;
            for (int d = 1; d < n; ++d) s = s + t0[-d * pitch - d];
            qf = s * a.rcp[n];
        }
        if (a.rev) {
            const int n = min(nr, nc_r);
            float s = s0;
            for (int d = 1; d < n; ++d) s = s + t0[-d * pitch + d];
            qr = s * a.rcp[n];
        }
        // both directions: reverse where it is larger or forward is NaN; forward wins ties
        const bool take_rev = a.rev && (!a.fwd || qr > qf || qf != qf);
        const float q = take_rev ? qr : qf;
        long long self = a.row0 + (long long)r;          // (uniform over the workgroup)
        if (a.row_self) {
            self = a.row_self[r];
            if (PASS == 1 && tx == 0 && tid == 0 && (self < 0 || self >= a.M)) atomicOr(a.status, 16);
        }
        int ea, eb;
        tk_bounds(self, a.window, a.causal, ea, eb);
        const bool hit = in && (c < ea || c > eb) && q >= a.thr;
        const unsigned long long B = __ballot(hit);
        const int64_t o = (int64_t)(r - a.ctx);
        if constexpr (PASS == 1) {
            if (lane == 0) a.seg[o * a.nseg + segment] = __popcll(B);
        } else if (B != 0ull) {                          // (a segment without a hit reads no offsets)
            const int64_t p = a.row_ptr[o] + a.seg[o * a.nseg + segment] + __popcll(B & below);
            if (hit && p < a.cap) {
                a.rows[p] = a.rout0 + (int)o;
                a.cols[p] = c;
                a.vals[p] = q;
                if (a.dirs) a.dirs[p] = take_rev ? 1 : 0;
            }
        }
    }
}

// seg[o][0 .. nseg) -> exclusive prefix sums in place, cnt[o] = the row's total; one wave per output row
__global__ __launch_bounds__(256) void seq_above_rowscan_kernel(int32_t* __restrict__ seg, int n, int nseg,
                                                                int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n) return;
    int32_t* p = seg + (int64_t)o * nseg;
    int run = 0;
    for (int j0 = 0; j0 < nseg; j0 += 64) {
        const int j = j0 + lane;
        const int v = j < nseg ? p[j] : 0;
        int x = v;                                       // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (j < nseg) p[j] = run + x - v;
        run += __shfl(x, 63);
    }
    if (lane == 0) cnt[o] = run;
}

int launch_seq_above_rowscan(int32_t* seg, int n, int nseg, int32_t* cnt, hipStream_t s) {
    hipLaunchKernelGGL(seq_above_rowscan_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, seg, n, nseg, cnt);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "seq_above_rowscan_kernel launch");
}

static size_t seq_a256(size_t v) { return (v + 255) & ~(size_t)255; }

// seg [n][ceil(M / 64)] i32 | cnt [n] i32
size_t seq_above_ws_bytes(int n, int M) {
    if (n <= 0 || M <= 0) return 0;
    return seq_a256((size_t)n * ((M + 63) / 64) * 4) + seq_a256((size_t)n * 4);
}

int launch_seq_above(const float* score, int R, int M, int64_t ld, int ctx, int L, int flags, const int32_t* row_self,
                     int row0, int window, int causal, float thr, int32_t* orows, int32_t* ocols, float* ovals,
                     unsigned char* odirs, int64_t cap, int64_t* row_ptr, int rout0, unsigned long long* count,
                     int accumulate, void* ws, int32_t* status, hipStream_t s) {
    const int n = R - ctx;
    if (n <= 0 || M <= 0) return SGPR_OK;
    static LdsLimitOnce once1, once2;
    const int lds_max = (SEQ_TR + SGPR_SEQ_MAX_LEN - 1) * (SEQ_TC + 2 * (SGPR_SEQ_MAX_LEN - 1)) * (int)sizeof(float);
    int rc = raise_lds_limit(&once1, reinterpret_cast<const void*>(seq_above_kernel<1>), lds_max,
                             "sequence range selection");
    if (rc != SGPR_OK) return rc;
    rc = raise_lds_limit(&once2, reinterpret_cast<const void*>(seq_above_kernel<2>), lds_max,
                         "sequence range selection");
    if (rc != SGPR_OK) return rc;
    SeqAboveArgs a;
    a.score = score;
    a.R = R;
    a.M = M;
    a.ld = ld;
    a.ctx = ctx;
    a.L = L;
    a.fwd = (flags & SGPR_SEQ_FORWARD) ? 1 : 0;
    a.rev = (flags & SGPR_SEQ_REVERSE) ? 1 : 0;
    a.nseg = (M + 63) / 64;
    a.row_self = row_self;
    a.row0 = row0;
    a.window = window;
    a.causal = causal;
    a.thr = thr;
    a.seg = static_cast<int32_t*>(ws);
    int32_t* cnt = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(ws) + seq_a256((size_t)n * a.nseg * 4));
    a.row_ptr = row_ptr;
    a.rout0 = rout0;
    a.rows = orows;
    a.cols = ocols;
    a.vals = ovals;
    a.dirs = odirs;
    a.cap = cap;
    a.status = status;
    a.rcp[0] = 0.f;
    for (int i = 1; i <= SGPR_SEQ_MAX_LEN; ++i) a.rcp[i] = (float)(1.0 / i);
    const int64_t tx = (M + SEQ_TC - 1) / SEQ_TC, ty = (n + SEQ_TR - 1) / SEQ_TR;
    if (tx * ty > 0x7fffffffLL) {
        set_error("sequence range selection: more than 2^31 tiles");
        return SGPR_E_INVALID;
    }
    a.tiles_x = (int)tx;
    const int rows = std::min(SEQ_TR, n);
    const size_t lds = (size_t)(rows + L - 1) * (SEQ_TC + 2 * (L - 1)) * sizeof(float);
    hipLaunchKernelGGL(seq_above_kernel<1>, dim3((unsigned)(tx * ty)), dim3(SEQ_TC), lds, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "seq_above_kernel launch (pass 1)");
    rc = launch_seq_above_rowscan(a.seg, n, a.nseg, cnt, s);
    if (rc != SGPR_OK) return rc;
    rc = launch_above_scan(cnt, n, row_ptr, count, accumulate, s);
    if (rc != SGPR_OK || cap == 0) return rc;              // (capacity 0: count only)
    hipLaunchKernelGGL(seq_above_kernel<2>, dim3((unsigned)(tx * ty)), dim3(SEQ_TC), lds, s, a);
    e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "seq_above_kernel launch (pass 2)");
}

// dirs[i] of a selected list: the direction at the selected column (dir block [n][ld]) or, one direction asked for, that
// direction; 0 in a padding slot (index -1)
__global__ __launch_bounds__(256) void seq_dirs_kernel(const int32_t* idx, int64_t total, int k, const unsigned char* dir,
                                                       int64_t ld, int fixed, unsigned char* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = idx[i];
    out[i] = c < 0 ? 0 : (dir ? dir[(i / k) * ld + c] : (unsigned char)fixed);
}

int launch_seq_dirs(const int32_t* idx, int n, int k, const unsigned char* dir, int64_t ld, int fixed,
                    unsigned char* out, hipStream_t s) {
    const int64_t total = (int64_t)n * k;
    if (total <= 0) return SGPR_OK;
    hipLaunchKernelGGL(seq_dirs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, idx, total, k, dir, ld,
                       fixed, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "seq_dirs_kernel launch");
}

}  // namespace sgpr

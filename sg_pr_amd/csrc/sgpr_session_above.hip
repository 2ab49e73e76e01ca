// Thresholded closures on multi-session maps (sgpr_session_rows_above, sgpr_score_session_above): the range selection of
// sgpr_seq_rows_above on the session-aware path-set score of sgpr_session_filter, with a minimum term count.
// DESIGN.md §23.
//
// S, the session tables, sess / lo / hi, D_p(r, c), Q_{p,sigma}, the additions, the multiplication and the session
// window are sgpr_session.hip's.  A candidate (p, sigma) takes part in the fold only when |D_p(r, c)| >= min_terms; the
// fold visits the participating candidates in session_kernel's order (paths ascending, forward before reverse, q > best
// || best != best) and the first of them initialises it.  An end point with no participating candidate is not eligible.
//
// session_above_kernel<FWD, REV, PASS> is session_kernel's tile - the 32 x 256 outputs, the (rows + L-1) x (256 + 2H)
// fp32 scores in dynamic LDS, the offsets as scalar words in the kernel arguments, the per-tile column-table walk, the
// uniform row-table walk and the inner d loop - with seq_above_kernel<PASS>'s range-select epilogue (sgpr_seq.hip) in
// place of the two stores: a thread owns a column, a wave a 64-column segment of the tile.
//   pass 1    per output row: hit = eligible && q >= thr, one ballot; lane 0 stores its popcount to seg[o][segment].
//             Exactly one wave writes every (o, segment) entry, zeros included: no memset, nothing read from before.
//   row scan, scan   seq_above_rowscan_kernel and above_scan_kernel, through their launchers.
//   pass 2    recomputes q (the same instructions): position = row_ptr[o] + seg[o][segment] + hits in the lanes below.
// A thread of the last tile whose column is >= M stays in the row loop with hit = false: its wave's count must be
// written (session_kernel returns there).  Plain vector stores; the only atomic is the status OR of a row_self entry
// outside [0, M), by one thread per row.
#include <algorithm>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int SA_TR = 32;     // output rows per tile
constexpr int SA_TC = 256;    // columns per tile = threads per workgroup
constexpr int SA_WORDS = SGPR_SEQ_MAX_LEN / 4;   // a path's offsets, four bytes to a word

struct SessionAboveArgs {
    const float* score;   // [R][ld]
    int R, M;
    int64_t ld;
    int ctx, L;
    int n_paths, H;       // H = the largest offset of the call
    int min_terms;        // 1..L
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
    unsigned char* codes; // or nullptr
    int64_t cap;
    int32_t* status;
    int n_row, n_col;     // sessions (>= 1)
    float rcp[SGPR_SEQ_MAX_LEN + 1];   // rcp[n] = (float)(1.0 / n), rounded once from double on the host
    uint32_t off[SGPR_SEQ_MAX_PATHS][SA_WORDS];   // byte d of path p: off_p[d]
    int32_t row_starts[SGPR_SESSION_MAX];
    int32_t col_starts[SGPR_SESSION_MAX];
};
static_assert(sizeof(SessionAboveArgs) < 4096, "the kernel arguments stay under 4 KB");

template <bool FWD, bool REV, int PASS>
__global__ __launch_bounds__(SA_TC) void session_above_kernel(const SessionAboveArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float sa_tile[];
    __shared__ float sa_rcp[SGPR_SEQ_MAX_LEN + 1];
    const int tid = threadIdx.x, h = a.L - 1, H = a.H;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int r_base = a.ctx + ty * SA_TR, c_base = tx * SA_TC;
    const int rows = min(SA_TR, a.R - r_base);           // output rows of this tile (>= 1 by the grid)
    const int pitch = SA_TC + 2 * H;
    if (tid <= SGPR_SEQ_MAX_LEN) sa_rcp[tid] = a.rcp[tid];
    // LDS row lr holds input row r_base - h + lr, LDS column lc input column c_base - H + lc
    for (int lr = 0; lr < rows + h; ++lr) {
        const int r = r_base - h + lr;                   // < R by construction
        const float* sp = a.score + (int64_t)(r < 0 ? 0 : r) * a.ld;
        for (int lc = tid; lc < pitch; lc += SA_TC) {
            const int c = c_base - H + lc;
            sa_tile[lr * pitch + lc] = (r >= 0 && c >= 0 && c < a.M) ? sp[c] : 0.f;
        }
    }
    __syncthreads();
    const int lane = tid & 63, segment = tx * (SA_TC / 64) + (tid >> 6);
    if (segment >= a.nseg) return;                       // (a whole wave beyond M: no segment of its own, no barrier ahead)
    const int c = c_base + tid;
    // a tail lane of the wave that holds column M - 1 stays for the ballots, never a hit; its words are inside the
    // tile's row (tid + H -+ o lies in 0 .. pitch - 1 for every tid) and hold staged zeros
    const bool in = c < a.M;
    // the lane's column session: its index, first and last column
    int sc = 0, lo = 0, hi = a.M - 1;
    for (int j = 1; j < a.n_col; ++j) {                  // (uniform trip count, a scalar load per step)
        const int s = a.col_starts[j];
        const bool le = s <= c;
        sc = le ? j : sc;
        lo = le ? s : lo;
        hi = (!le && s - 1 < hi) ? s - 1 : hi;           // the first start past c ends the session (starts ascend)
    }
    const int room_f = c - lo, room_r = hi - c;          // the largest offset a forward / reverse term may take
    const unsigned long long below = (1ull << lane) - 1ull;
    int jr = 0;                                          // the row session of the tile's current row (uniform)
    for (int i = 0; i < rows; ++i) {
        const int r = r_base + i;
        while (jr + 1 < a.n_row && a.row_starts[jr + 1] <= r) ++jr;
        const float* t0 = sa_tile + (i + h) * pitch + H + tid;
        const int nr = min(a.L, r - a.row_starts[jr] + 1);
        const float s0 = t0[0];
        float bf = 0.f, br = 0.f;
        int cf = 0, cr = 1;
        bool have_f = false, have_r = false;
        for (int p = 0; p < a.n_paths; ++p) {
            uint32_t w[SA_WORDS];                        // the path's offsets: wave-uniform, indexed by constants below
#pragma unroll
            for (int j = 0; j < SA_WORDS; ++j) w[j] = a.off[p][j];
            float sf = s0, sr = s0;
            int nf = 1, nb = 1;
#pragma unroll
            for (int d = 1; d < SGPR_SEQ_MAX_LEN; ++d) {
                if (d >= nr) break;                      // (uniform)
                const int o = (int)((w[d >> 2] >> (8 * (d & 3))) & 0xffu);
                const float* t = t0 - d * pitch;
                if (FWD) {
                    const float v = t[-o];
                    const bool inside = o <= room_f;
                    sf = inside ? sf + v : sf;
                    nf += inside ? 1 : 0;
                }
                if (REV) {
                    const float v = t[o];
                    const bool inside = o <= room_r;
                    sr = inside ? sr + v : sr;
                    nb += inside ? 1 : 0;
                }
            }
            if (FWD) {
                const float q = sf * sa_rcp[nf];
                if (nf >= a.min_terms && (!have_f || q > bf || bf != bf)) {
                    bf = q;
                    cf = p << 1;
                    have_f = true;
                }
            }
            if (REV) {
                const float q = sr * sa_rcp[nb];
                if (nb >= a.min_terms && (!have_r || q > br || br != br)) {
                    br = q;
                    cr = (p << 1) | 1;
                    have_r = true;
                }
            }
        }
        // both directions: reverse where it is larger or forward is NaN or absent; forward wins ties
        const bool take_rev = have_r && (!have_f || br > bf || bf != bf);
        const float q = take_rev ? br : bf;
        const int cd = take_rev ? cr : cf;
        long long self = a.row0 + (long long)r;          // (uniform over the workgroup)
        if (a.row_self) {
            self = a.row_self[r];
            if (PASS == 1 && tx == 0 && tid == 0 && (self < 0 || self >= a.M)) atomicOr(a.status, 16);
        }
        bool excluded = false;
        if (a.window >= 0) {                             // (uniform) the session window, on the end point alone
            int ss = 0;
            for (int j = 1; j < a.n_col; ++j) ss = a.col_starts[j] <= self ? j : ss;   // (self < 0: session 0)
            const long long dist = (long long)c - self;
            excluded = ss == sc && (dist < 0 ? -dist : dist) <= (long long)a.window;
        }
        int ea, eb;
        tk_bounds(self, -1, a.causal, ea, eb);           // (causal: c < self; the window above is the session's)
        const bool hit = in && (have_f || have_r) && !excluded && c < ea && q >= a.thr;
        const unsigned long long B = __ballot(hit);
        const int64_t o = (int64_t)(r - a.ctx);
        if constexpr (PASS == 1) {
            if (lane == 0) a.seg[o * a.nseg + segment] = __popcll(B);
        } else if (B != 0ull) {                          // (a segment without a hit reads no offsets)
            const int64_t pos = a.row_ptr[o] + a.seg[o * a.nseg + segment] + __popcll(B & below);
            if (hit && pos < a.cap) {
                a.rows[pos] = a.rout0 + (int)o;
                a.cols[pos] = c;
                a.vals[pos] = q;
                if (a.codes) a.codes[pos] = (unsigned char)cd;
            }
        }
    }
}

template <bool FWD, bool REV, int PASS>
static int launch_session_above_pass(const SessionAboveArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
    static LdsLimitOnce once;
    const int lds_max = (SA_TR + SGPR_SEQ_MAX_LEN - 1) * (SA_TC + 2 * SGPR_SEQ_PATH_MAX_OFFSET) * (int)sizeof(float);
    const int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(session_above_kernel<FWD, REV, PASS>), lds_max,
                                   "session range selection");
    if (rc != SGPR_OK) return rc;
    hipLaunchKernelGGL((session_above_kernel<FWD, REV, PASS>), dim3(blocks), dim3(SA_TC), lds, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK
                           : hip_fail(e, PASS == 1 ? "session_above_kernel launch (pass 1)"
                                                   : "session_above_kernel launch (pass 2)");
}

template <int PASS>
static int launch_session_above_dir(const SessionAboveArgs& a, int flags, unsigned blocks, size_t lds, hipStream_t s) {
    const bool fwd = (flags & SGPR_SEQ_FORWARD) != 0, rev = (flags & SGPR_SEQ_REVERSE) != 0;
    if (fwd && rev) return launch_session_above_pass<true, true, PASS>(a, blocks, lds, s);
    return fwd ? launch_session_above_pass<true, false, PASS>(a, blocks, lds, s)
               : launch_session_above_pass<false, true, PASS>(a, blocks, lds, s);
}

// arguments already checked (launch_session_filter's and launch_seq_above's, min_terms in 1..L)
int launch_session_above(const float* score, int R, int M, int64_t ld, int ctx, int L, int flags, const int32_t* offsets,
                         int n_paths, const int32_t* row_starts, int n_row, const int32_t* col_starts, int n_col,
                         const int32_t* row_self, int row0, int window, int causal, int min_terms, float thr,
                         int32_t* orows, int32_t* ocols, float* ovals, unsigned char* ocodes, int64_t cap,
                         int64_t* row_ptr, int rout0, unsigned long long* count, int accumulate, void* ws, int32_t* status,
                         hipStream_t s) {
    const int n = R - ctx;
    if (n <= 0 || M <= 0) return SGPR_OK;
    SessionAboveArgs a;
    a.score = score;
    a.R = R;
    a.M = M;
    a.ld = ld;
    a.ctx = ctx;
    a.L = L;
    a.n_paths = offsets ? n_paths : 1;
    a.H = 0;
    for (int p = 0; p < SGPR_SEQ_MAX_PATHS; ++p) {
        for (int j = 0; j < SA_WORDS; ++j) a.off[p][j] = 0u;
        for (int d = 0; p < a.n_paths && d < L; ++d) {
            const int o = offsets ? offsets[(size_t)p * L + d] : d;
            a.off[p][d >> 2] |= (uint32_t)o << (8 * (d & 3));
            a.H = std::max(a.H, o);
        }
    }
    a.min_terms = min_terms;
    a.nseg = (M + 63) / 64;
    a.row_self = row_self;
    a.row0 = row0;
    a.window = window;
    a.causal = causal;
    a.thr = thr;
    a.seg = static_cast<int32_t*>(ws);
    // seg [n][nseg] i32 | cnt [n] i32 (seq_above_ws_bytes)
    int32_t* cnt = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(ws) +
                                              (((size_t)n * a.nseg * 4 + 255) & ~(size_t)255));
    a.row_ptr = row_ptr;
    a.rout0 = rout0;
    a.rows = orows;
    a.cols = ocols;
    a.vals = ovals;
    a.codes = ocodes;
    a.cap = cap;
    a.status = status;
    a.n_row = row_starts ? n_row : 1;
    a.n_col = col_starts ? n_col : 1;
    for (int j = 0; j < SGPR_SESSION_MAX; ++j) {
        a.row_starts[j] = row_starts && j < n_row ? row_starts[j] : (j == 0 ? 0 : R);
        a.col_starts[j] = col_starts && j < n_col ? col_starts[j] : (j == 0 ? 0 : M);
    }
    a.rcp[0] = 0.f;
    for (int i = 1; i <= SGPR_SEQ_MAX_LEN; ++i) a.rcp[i] = (float)(1.0 / i);
    const int64_t tx = (M + SA_TC - 1) / SA_TC, ty = (n + SA_TR - 1) / SA_TR;
    if (tx * ty > 0x7fffffffLL) {
        set_error("session range selection: more than 2^31 tiles");
        return SGPR_E_INVALID;
    }
    a.tiles_x = (int)tx;
    const int rows = std::min(SA_TR, n);
    const size_t lds = (size_t)(rows + L - 1) * (SA_TC + 2 * a.H) * sizeof(float);
    int rc = launch_session_above_dir<1>(a, flags, (unsigned)(tx * ty), lds, s);
    if (rc != SGPR_OK) return rc;
    rc = launch_seq_above_rowscan(a.seg, n, a.nseg, cnt, s);
    if (rc != SGPR_OK) return rc;
    rc = launch_above_scan(cnt, n, row_ptr, count, accumulate, s);
    if (rc != SGPR_OK || cap == 0) return rc;              // (capacity 0: count only)
    return launch_session_above_dir<2>(a, flags, (unsigned)(tx * ty), lds, s);
}

}  // namespace sgpr

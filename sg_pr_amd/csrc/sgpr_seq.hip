// The sequence-matching family: the mean of the scores along a diagonal, or along the best of a set of paths, of the
// similarity matrix that ends in (r, c) - stored (sgpr_seq_filter, sgpr_seq_path_filter, sgpr_session_filter and the
// ranking calls on them) or range-selected (sgpr_seq_rows_above, sgpr_session_rows_above and the pooled forms).
// DESIGN.md §17, §18, §21, §22, §23; the pieces and who instantiates which: the end of §23.
//
// A path is off[0..L-1], off[0] = 0, non-decreasing, off[L-1] <= SGPR_SEQ_PATH_MAX_OFFSET: the column distance walked
// back after d row steps (off[d] = d is the unit diagonal).  For path p and sigma = +1 forward, -1 reverse:
//
//   D_p(r, c)    = { d in 0..L-1 : r - d >= lo_row(r) and lo_col(c) <= c - sigma off_p[d] <= hi_col(c) }
//   Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|]         fp32 additions in ascending d
//
// lo / hi are the edges of the matrix or, with session tables, of the session that holds r or c (starts[0] = 0,
// non-decreasing, a repeated value is an empty session; sess(x) = the largest j with starts[j] <= x, x < 0: session 0).
// Every condition is monotone in d (off is), so D is a prefix: a lane runs its own trip count (unit diagonal) or drops
// the terms past its room by a select (path set).  No term is ever masked or replaced by a zero - a zero would turn a
// -0.0 sum into +0.0.  The output is a fold over the candidates, forward paths 0..P-1 and then reverse paths 0..P-1:
// best starts as the first candidate, a later x replaces it iff x > best or best is NaN; code = direction bit |
// path << 1 of the winner.  With min_terms a candidate takes part only when |D_p| >= min_terms, the first participant
// initialises the fold, and an end point without one is not eligible.  The session window excludes the end point (r, c)
// iff sess_col(c) == sess_col(self_r) and |c - self_r| <= window (self_r = row_self[r] or row0 + r).
//
// One workgroup per tile of SEQ_TR output rows x SEQ_TC columns.  It stages the (rows + L-1) x (SEQ_TC + 2H) scores its
// walks reach into LDS (H = L - 1 for the unit diagonal, the call's largest offset for a path set: 80 136 bytes at
// L = 32, 96 768 at H = 64) - lanes along a row, so every global load is a contiguous run, zero outside the rectangle -
// and then each thread owns one column and walks the tile's rows.  At step d lane i reads word (row - d) * pitch + i -+
// off[d]: adjacent lanes, adjacent words, in either direction and for every path (no bank conflict).
//
// Each __global__ below is a thin instantiation of unit_tile<PASS> or path_tile<FWD, REV, SESS, PASS>; everything that
// differs between them is `if constexpr`, so no kernel carries another's arguments or branches.  unit_tile is built
// from small helpers; path_tile shares the staging with it and is otherwise written in one piece: cut into helpers
// (walk, bounds, range-select epilogue) its kernels compiled to a different schedule and, in pass 1, two more SGPRs,
// and measured 0.3 - 1.9 % slower than their hand-written predecessors (the end of §23).
#include <algorithm>
#include <type_traits>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int SEQ_TR = 32;     // output rows per tile
constexpr int SEQ_TC = 256;    // columns per tile = threads per workgroup
constexpr int SEQ_WORDS = SGPR_SEQ_MAX_LEN / 4;   // a path's offsets, four bytes to a word

// ------------------------------------------------------------------ kernel arguments
struct TileArgs {          // the common prefix
    const float* score;   // [R][ld]
    int R, M;
    int64_t ld;
    int ctx, L;
};

struct PathTable {
    float rcp[SGPR_SEQ_MAX_LEN + 1];   // rcp[n] = (float)(1.0 / n), rounded once from double on the host
    uint32_t off[SGPR_SEQ_MAX_PATHS][SEQ_WORDS];   // byte d of path p: off_p[d]
};

struct RangeArgs {         // the range-select epilogue's
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
};

struct SeqArgs : TileArgs {
    int fwd, rev;
    float* out;           // [R - ctx][ldo]
    int64_t ldo;
    unsigned char* code;  // [R - ctx][ldc] or nullptr: the direction taken
    int64_t ldc;
    int tiles_x;
    float rcp[SGPR_SEQ_MAX_LEN + 1];
};

struct SeqAboveArgs : TileArgs {
    int fwd, rev;
    int tiles_x, nseg;    // nseg = ceil(M / 64)
    RangeArgs rg;
    float rcp[SGPR_SEQ_MAX_LEN + 1];
};

struct SeqPathArgs : TileArgs {
    int n_paths, H;       // H = the largest offset of the call
    float* out;
    int64_t ldo;
    unsigned char* code;
    int64_t ldc;
    int tiles_x;
    PathTable pt;
};

struct SessionArgs : TileArgs {
    int n_paths, H;
    float* out;
    int64_t ldo;
    unsigned char* code;
    int64_t ldc;
    const int32_t* row_self;   // [R] or nullptr: row0 + r
    int row0, window;
    int tiles_x;
    int n_row, n_col;     // sessions (>= 1)
    PathTable pt;
    int32_t row_starts[SGPR_SESSION_MAX];
    int32_t col_starts[SGPR_SESSION_MAX];
};
static_assert(sizeof(SessionArgs) < 4096, "the kernel arguments stay under 4 KB");

struct SessionAboveArgs : TileArgs {
    int n_paths, H;
    int min_terms;        // 1..L
    int tiles_x, nseg;
    RangeArgs rg;
    int n_row, n_col;
    PathTable pt;
    int32_t row_starts[SGPR_SESSION_MAX];
    int32_t col_starts[SGPR_SESSION_MAX];
};
static_assert(sizeof(SessionAboveArgs) < 4096, "the kernel arguments stay under 4 KB");

// ------------------------------------------------------------------ device pieces
extern __shared__ float seq_tile[];

struct Tile {
    int tid, tx, r_base, c_base;
    int rows;             // output rows of this tile (>= 1 by the grid)
    int h, H, pitch;      // LDS row lr holds input row r_base - h + lr, LDS column lc input column c_base - H + lc
    __device__ const float* at(int i) const { return seq_tile + (i + h) * pitch + H + tid; }   // output row i, own column
};

template <class A>
__device__ __forceinline__ Tile tile_of(const A& a, int H) {
    Tile t;
    t.tid = threadIdx.x;
    t.h = a.L - 1;
    t.H = H;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
    t.tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    t.r_base = a.ctx + ty * SEQ_TR;
    t.c_base = t.tx * SEQ_TC;
    t.rows = min(SEQ_TR, a.R - t.r_base);
    t.pitch = SEQ_TC + 2 * H;
    return t;
}

template <class A>
__device__ __forceinline__ void stage_tile(const A& a, const Tile& t) {
    for (int lr = 0; lr < t.rows + t.h; ++lr) {
        const int r = t.r_base - t.h + lr;               // < R by construction
        const float* sp = a.score + (int64_t)(r < 0 ? 0 : r) * a.ld;
        for (int lc = t.tid; lc < t.pitch; lc += SEQ_TC) {
            const int c = t.c_base - t.H + lc;
            seq_tile[lr * t.pitch + lc] = (r >= 0 && c >= 0 && c < a.M) ? sp[c] : 0.f;
        }
    }
    __syncthreads();
}

struct Best {              // an end point's score and the direction taken
    float q;
    int code;
};

// a reverse candidate beside the forward one: reverse where it is larger or forward is NaN or absent; forward wins ties
__device__ __forceinline__ bool join_rev(bool have_f, float qf, float qr) {
    return !have_f || qr > qf || qf != qf;
}

// the unit diagonal: D is the prefix 0..n-1, n = min(L, depth, c + 1) forward or min(L, depth, M - c) reverse
template <class A>
__device__ __forceinline__ Best unit_walk(const A& a, const float* t0, int pitch, int nr, int nc_f, int nc_r) {
#pragma clang fp contract(off)
    const float s0 = t0[0];
    float qf = 0.f, qr = 0.f;
    bool take_rev = false;
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
        take_rev = join_rev(a.fwd, qf, qr);
    }
    return {take_rev ? qr : qf, take_rev ? 1 : 0};
}

// Epilogue 1: store Q and the code.
template <class A>
__device__ __forceinline__ void store_end(const A& a, int64_t o, int c, float q, int cd) {
    a.out[o * a.ldo + c] = q;
    if (a.code) a.code[o * a.ldc + c] = (unsigned char)cd;
}

// Epilogue 2: range selection.  A thread owns a column, a wave a 64-column segment of the tile.
//   pass 1    per output row: hit = eligible && q >= thr, one ballot; lane 0 stores its popcount to seg[o][segment].
//             Exactly one wave writes every (o, segment) entry, zeros included: no memset, nothing read from before.
//   row scan  seq_above_rowscan_kernel, one wave per output row: seg[o][*] -> exclusive offsets in place, cnt[o].
//   scan      above_scan_kernel (sgpr_score.hip): cnt -> row_ptr and the running total, continuing across row blocks.
//   pass 2    recomputes q (the same instructions): position = row_ptr[o] + seg[o][segment] + hits in the lanes below.
// A tail lane of the wave that holds column M - 1 stays in the row loop for the ballots, never a hit: its words are
// inside the tile's row and hold staged zeros.  Plain vector stores; the only atomic is the status OR of a row_self
// entry outside [0, M) (rows_above_kernel's bit), by one thread per row in pass 1.
template <int PASS>
__device__ __forceinline__ long long range_self(const RangeArgs& g, int M, int r, int tx, int tid) {
    long long self = g.row0 + (long long)r;              // (uniform over the workgroup)
    if (g.row_self) {
        self = g.row_self[r];
        if (PASS == 1 && tx == 0 && tid == 0 && (self < 0 || self >= M)) atomicOr(g.status, 16);
    }
    return self;
}

template <int PASS>
__device__ __forceinline__ void range_select(const RangeArgs& g, int nseg, int lane, int segment,
                                             unsigned long long below, int64_t o, int c, bool hit, float q, int cd) {
    const unsigned long long B = __ballot(hit);
    if constexpr (PASS == 1) {
        if (lane == 0) g.seg[o * nseg + segment] = __popcll(B);
    } else if (B != 0ull) {                              // (a segment without a hit reads no offsets)
        const int64_t p = g.row_ptr[o] + g.seg[o * nseg + segment] + __popcll(B & below);
        if (hit && p < g.cap) {
            g.rows[p] = g.rout0 + (int)o;
            g.cols[p] = c;
            g.vals[p] = q;
            if (g.codes) g.codes[p] = (unsigned char)cd;
        }
    }
}

// PASS 0: store; 1, 2: range selection
template <int PASS, class A>
__device__ __forceinline__ void unit_tile(const A& a) {
#pragma clang fp contract(off)
    const Tile t = tile_of(a, a.L - 1);
    stage_tile(a, t);
    const int lane = t.tid & 63, segment = t.tx * (SEQ_TC / 64) + (t.tid >> 6);
    if constexpr (PASS > 0) {
        if (segment >= a.nseg) return;                   // (a whole wave beyond M: no segment of its own, no barrier ahead)
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const int c = t.c_base + t.tid;
    const bool in = c < a.M;
    if constexpr (PASS == 0) {
        if (!in) return;
    }
    const int nc_f = in ? min(a.L, c + 1) : 1, nc_r = in ? min(a.L, a.M - c) : 1;
    for (int i = 0; i < t.rows; ++i) {
        const int r = t.r_base + i;
        const Best b = unit_walk(a, t.at(i), t.pitch, min(a.L, r + 1), nc_f, nc_r);
        if constexpr (PASS == 0) {
            store_end(a, (int64_t)(r - a.ctx), c, b.q, b.code);
        } else {
            const long long self = range_self<PASS>(a.rg, a.M, r, t.tx, t.tid);
            int ea, eb;
            tk_bounds(self, a.rg.window, a.rg.causal, ea, eb);
            const bool hit = in && (c < ea || c > eb) && b.q >= a.rg.thr;
            range_select<PASS>(a.rg, a.nseg, lane, segment, below, (int64_t)(r - a.ctx), c, hit, b.q, b.code);
        }
    }
}

// The path set: one body, written in one piece (see DESIGN §23 on why it is not cut into helper functions).
// SESS: session tables bound the rooms and the depth, and the session window applies.  PASS 0: store; 1, 2: range
// selection with the minimum term count.  rcp[] sits in 33 words of static LDS.
template <bool FWD, bool REV, bool SESS, int PASS, class A>
__device__ __forceinline__ void path_tile(const A& a) {
#pragma clang fp contract(off)
    __shared__ float rcp[SGPR_SEQ_MAX_LEN + 1];
    const Tile t = tile_of(a, a.H);
    const int tid = t.tid, tx = t.tx, r_base = t.r_base, c_base = t.c_base, rows = t.rows, h = t.h, H = t.H, pitch = t.pitch;
    if (tid <= SGPR_SEQ_MAX_LEN) rcp[tid] = a.pt.rcp[tid];
    stage_tile(a, t);
    const int lane = tid & 63, segment = tx * (SEQ_TC / 64) + (tid >> 6);
    if constexpr (PASS > 0) {
        if (segment >= a.nseg) return;                   // (a whole wave beyond M: no segment of its own, no barrier ahead)
    }
    const int c = c_base + tid;
    if constexpr (PASS == 0) {
        if (c >= a.M) return;
    }
    // PASS > 0: a tail lane of the wave that holds column M - 1 stays for the ballots, never a hit; its words are inside
    // the tile's row (tid + H -+ o lies in 0 .. pitch - 1 for every tid) and hold staged zeros
    const bool in = c < a.M;
    // the lane's column session: its index, first and last column
    int sc = 0, lo = 0, hi = a.M - 1;
    if constexpr (SESS) {
        for (int j = 1; j < a.n_col; ++j) {              // (uniform trip count, a scalar load per step)
            const int s = a.col_starts[j];
            const bool le = s <= c;
            sc = le ? j : sc;
            lo = le ? s : lo;
            hi = (!le && s - 1 < hi) ? s - 1 : hi;       // the first start past c ends the session (starts ascend)
        }
    }
    const int room_f = c - lo, room_r = hi - c;          // the largest offset a forward / reverse term may take
    const unsigned long long below = (1ull << lane) - 1ull;
    int jr = 0;                                          // the row session of the tile's current row (uniform)
    for (int i = 0; i < rows; ++i) {
        const int r = r_base + i;
        int depth = r + 1;
        if constexpr (SESS) {
            while (jr + 1 < a.n_row && a.row_starts[jr + 1] <= r) ++jr;
            depth = r - a.row_starts[jr] + 1;
        }
        const float* t0 = seq_tile + (i + h) * pitch + H + tid;
        const int nr = min(a.L, depth);
        const float s0 = t0[0];
        float bf = 0.f, br = 0.f;
        int cf = 0, cr = 1;
        bool have_f = PASS == 0 && FWD, have_r = PASS == 0 && REV;   // (PASS 0: every candidate takes part)
        for (int p = 0; p < a.n_paths; ++p) {
            uint32_t w[SEQ_WORDS];                       // the path's offsets: wave-uniform, indexed by constants below
#pragma unroll
            for (int j = 0; j < SEQ_WORDS; ++j) w[j] = a.pt.off[p][j];
            float sf = s0, sr = s0;
            int nf = 1, nb = 1;
            // A lane's terms are the prefix off_p[d] <= room.  Past it the word read is still inside the tile's row
            // (o <= H) and is dropped by the select: the sum keeps its bits, nothing is added in its place.
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
            // the two folds run side by side; PASS > 0: only candidates with at least min_terms terms, the first of
            // them initialises the fold
            if (FWD) {
                const float q = sf * rcp[nf];
                if constexpr (PASS == 0) {
                    if (p == 0 || q > bf || bf != bf) {
                        bf = q;
                        cf = p << 1;
                    }
                } else if (nf >= a.min_terms && (!have_f || q > bf || bf != bf)) {
                    bf = q;
                    cf = p << 1;
                    have_f = true;
                }
            }
            if (REV) {
                const float q = sr * rcp[nb];
                if constexpr (PASS == 0) {
                    if (p == 0 || q > br || br != br) {
                        br = q;
                        cr = (p << 1) | 1;
                    }
                } else if (nb >= a.min_terms && (!have_r || q > br || br != br)) {
                    br = q;
                    cr = (p << 1) | 1;
                    have_r = true;
                }
            }
        }
        // joined: that is the fold over "forward paths, then reverse paths"
        const bool take_rev = have_r && (!have_f || br > bf || bf != bf);   // (join_rev's rule, in place)
        float q = take_rev ? br : bf;
        int cd = take_rev ? cr : cf;
        const int64_t o = (int64_t)(r - a.ctx);
        if constexpr (PASS == 0) {
            if constexpr (SESS) {
                if (a.window >= 0) {                     // (uniform) the session window, on the end point alone
                    const int self = a.row_self ? __builtin_amdgcn_readfirstlane(a.row_self[r]) : a.row0 + r;
                    int ss = 0;
                    for (int j = 1; j < a.n_col; ++j) ss = a.col_starts[j] <= self ? j : ss;   // (self < 0: session 0)
                    const int64_t dist = (int64_t)c - (int64_t)self;
                    if (ss == sc && (dist < 0 ? -dist : dist) <= (int64_t)a.window) {
                        q = -__builtin_inff();
                        cd = 0;
                    }
                }
            }
            a.out[o * a.ldo + c] = q;
            if (a.code) a.code[o * a.ldc + c] = (unsigned char)cd;
        } else {
            long long self = a.rg.row0 + (long long)r;   // (uniform over the workgroup)
            if (a.rg.row_self) {
                self = a.rg.row_self[r];
                if (PASS == 1 && tx == 0 && tid == 0 && (self < 0 || self >= a.M)) atomicOr(a.rg.status, 16);
            }
            bool excluded = false;
            if (a.rg.window >= 0) {                      // (uniform) the session window, on the end point alone
                int ss = 0;
                for (int j = 1; j < a.n_col; ++j) ss = a.col_starts[j] <= self ? j : ss;   // (self < 0: session 0)
                const long long dist = (long long)c - self;
                excluded = ss == sc && (dist < 0 ? -dist : dist) <= (long long)a.rg.window;
            }
            int ea, eb;
            tk_bounds(self, -1, a.rg.causal, ea, eb);    // (causal: c < self; the window above is the session's)
            const bool hit = in && (have_f || have_r) && !excluded && c < ea && q >= a.rg.thr;
            const unsigned long long B = __ballot(hit);
            if constexpr (PASS == 1) {
                if (lane == 0) a.rg.seg[o * a.nseg + segment] = __popcll(B);
            } else if (B != 0ull) {                      // (a segment without a hit reads no offsets)
                const int64_t pos = a.rg.row_ptr[o] + a.rg.seg[o * a.nseg + segment] + __popcll(B & below);
                if (hit && pos < a.rg.cap) {
                    a.rg.rows[pos] = a.rg.rout0 + (int)o;
                    a.rg.cols[pos] = c;
                    a.rg.vals[pos] = q;
                    if (a.rg.codes) a.rg.codes[pos] = (unsigned char)cd;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ the entry points
__global__ __launch_bounds__(SEQ_TC) void seq_filter_kernel(const SeqArgs a) { unit_tile<0>(a); }

template <int PASS>
__global__ __launch_bounds__(SEQ_TC) void seq_above_kernel(const SeqAboveArgs a) {
    unit_tile<PASS>(a);
}

// FWD / REV: the directions asked for (at least one)
template <bool FWD, bool REV>
__global__ __launch_bounds__(SEQ_TC) void seq_path_kernel(const SeqPathArgs a) {
    path_tile<FWD, REV, false, 0>(a);
}

template <bool FWD, bool REV>
__global__ __launch_bounds__(SEQ_TC) void session_kernel(const SessionArgs a) {
    path_tile<FWD, REV, true, 0>(a);
}

template <bool FWD, bool REV, int PASS>
__global__ __launch_bounds__(SEQ_TC) void session_above_kernel(const SessionAboveArgs a) {
    path_tile<FWD, REV, true, PASS>(a);
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

// dirs[i] of a selected list: the direction at the selected column (dir block [n][ld]) or, one direction asked for, that
// direction; 0 in a padding slot (index -1)
__global__ __launch_bounds__(256) void seq_dirs_kernel(const int32_t* idx, int64_t total, int k, const unsigned char* dir,
                                                       int64_t ld, int fixed, unsigned char* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = idx[i];
    out[i] = c < 0 ? 0 : (dir ? dir[(i / k) * ld + c] : (unsigned char)fixed);
}

// ------------------------------------------------------------------ host side: the argument blocks
struct Grid {
    unsigned blocks;
    size_t lds;           // dynamic LDS bytes
};

static void fill_rcp(float* rcp) {
    rcp[0] = 0.f;
    for (int n = 1; n <= SGPR_SEQ_MAX_LEN; ++n) rcp[n] = (float)(1.0 / n);
}

// the common prefix, the grid and the tile's LDS for a halo of H columns either side
template <class A>
static int fill_tile(A& a, const ScoreBlock& b, const SeqSpec& seq, int H, const char* what, Grid* g) {
    a.score = b.score;
    a.R = b.R;
    a.M = b.M;
    a.ld = b.ld;
    a.ctx = seq.ctx;
    a.L = seq.L;
    const int64_t tx = (b.M + SEQ_TC - 1) / SEQ_TC, ty = (b.R - seq.ctx + SEQ_TR - 1) / SEQ_TR;
    if (tx * ty > 0x7fffffffLL) {
        set_error(std::string(what) + ": more than 2^31 tiles");
        return SGPR_E_INVALID;
    }
    a.tiles_x = (int)tx;
    g->blocks = (unsigned)(tx * ty);
    g->lds = (size_t)(std::min(SEQ_TR, b.R - seq.ctx) + seq.L - 1) * (SEQ_TC + 2 * H) * sizeof(float);
    return SGPR_OK;
}

// seq.offsets [n_paths][L] packed into bytes (already checked; nullptr: the unit diagonal), H and rcp
template <class A>
static void fill_paths(A& a, const SeqSpec& seq) {
    a.n_paths = seq.offsets ? seq.n_paths : 1;
    a.H = 0;
    for (int p = 0; p < SGPR_SEQ_MAX_PATHS; ++p) {
        for (int j = 0; j < SEQ_WORDS; ++j) a.pt.off[p][j] = 0u;
        for (int d = 0; p < a.n_paths && d < seq.L; ++d) {
            const int o = seq.offsets ? seq.offsets[(size_t)p * seq.L + d] : d;
            a.pt.off[p][d >> 2] |= (uint32_t)o << (8 * (d & 3));
            a.H = std::max(a.H, o);
        }
    }
    fill_rcp(a.pt.rcp);
}

// the two session tables (already checked: 1..64 entries, the first 0, non-decreasing, <= R / <= M; nullptr: one session)
template <class A>
static void fill_sessions(A& a, const SeqSpec& seq, int R, int M) {
    a.n_row = seq.row_starts ? seq.n_row : 1;
    a.n_col = seq.col_starts ? seq.n_col : 1;
    for (int j = 0; j < SGPR_SESSION_MAX; ++j) {
        a.row_starts[j] = seq.row_starts && j < seq.n_row ? seq.row_starts[j] : (j == 0 ? 0 : R);
        a.col_starts[j] = seq.col_starts && j < seq.n_col ? seq.col_starts[j] : (j == 0 ? 0 : M);
    }
}

// where a filter writes
template <class A>
static void fill_out(A& a, const FilterOut& o) {
    a.out = o.out;
    a.ldo = o.ldo;
    a.code = o.code;
    a.ldc = o.ldc;
}

// one instantiation: its LDS limit raised once (halo_max: the largest halo it can be asked for), then the launch
template <auto Kernel, class A>
static int launch_tile(const A& a, const Grid& g, int halo_max, const char* what, const char* fail, hipStream_t s) {
    static LdsLimitOnce once;
    const int lds_max = (SEQ_TR + SGPR_SEQ_MAX_LEN - 1) * (SEQ_TC + 2 * halo_max) * (int)sizeof(float);
    const int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(Kernel), lds_max, what);
    if (rc != SGPR_OK) return rc;
    hipLaunchKernelGGL(Kernel, dim3(g.blocks), dim3(SEQ_TC), g.lds, s, a);
    return launched(fail);
}

// f(FWD, REV) with the directions of `dirs` as compile-time constants
template <class F>
static int by_direction(int dirs, F&& f) {
    const bool fwd = (dirs & SGPR_SEQ_FORWARD) != 0, rev = (dirs & SGPR_SEQ_REVERSE) != 0;
    if (fwd && rev) return f(std::true_type{}, std::true_type{});
    return fwd ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::true_type{});
}

// ------------------------------------------------------------------ the filters
int launch_seq_filter(const ScoreBlock& b, const SeqSpec& seq, const FilterOut& out, hipStream_t s) {
    if (b.R - seq.ctx <= 0 || b.M <= 0) return SGPR_OK;
    SeqArgs a;
    Grid g;
    const int rc = fill_tile(a, b, seq, seq.L - 1, "sequence filter", &g);
    if (rc != SGPR_OK) return rc;
    a.fwd = (seq.dirs & SGPR_SEQ_FORWARD) ? 1 : 0;
    a.rev = (seq.dirs & SGPR_SEQ_REVERSE) ? 1 : 0;
    fill_out(a, out);
    fill_rcp(a.rcp);
    return launch_tile<seq_filter_kernel>(a, g, SGPR_SEQ_MAX_LEN - 1, "sequence filter", "seq_filter_kernel launch", s);
}

// arguments already checked (paths: off[p][0] = 0, non-decreasing, <= SGPR_SEQ_PATH_MAX_OFFSET; 1 <= n_paths <= 16)
int launch_seq_path_filter(const ScoreBlock& b, const SeqSpec& seq, const FilterOut& out, hipStream_t s) {
    if (b.R - seq.ctx <= 0 || b.M <= 0) return SGPR_OK;
    SeqPathArgs a;
    Grid g;
    fill_paths(a, seq);
    const int rc = fill_tile(a, b, seq, a.H, "sequence path filter", &g);
    if (rc != SGPR_OK) return rc;
    fill_out(a, out);
    return by_direction(seq.dirs, [&](auto F, auto V) {
        return launch_tile<seq_path_kernel<decltype(F)::value, decltype(V)::value>>(
            a, g, SGPR_SEQ_PATH_MAX_OFFSET, "sequence path filter", "seq_path_kernel launch", s);
    });
}

// arguments already checked (paths as launch_seq_path_filter's, offsets == nullptr: the unit diagonal; tables: see
// fill_sessions)
int launch_session_filter(const ScoreBlock& b, const SeqSpec& seq, const Eligible& e, const FilterOut& out,
                          hipStream_t s) {
    if (b.R - seq.ctx <= 0 || b.M <= 0) return SGPR_OK;
    SessionArgs a;
    Grid g;
    fill_paths(a, seq);
    const int rc = fill_tile(a, b, seq, a.H, "session filter", &g);
    if (rc != SGPR_OK) return rc;
    fill_sessions(a, seq, b.R, b.M);
    fill_out(a, out);
    a.row_self = e.row_self;
    a.row0 = e.row0;
    a.window = e.window;
    return by_direction(seq.dirs, [&](auto F, auto V) {
        return launch_tile<session_kernel<decltype(F)::value, decltype(V)::value>>(
            a, g, SGPR_SEQ_PATH_MAX_OFFSET, "session filter", "session_kernel launch", s);
    });
}

// ------------------------------------------------------------------ range selection
int launch_seq_above_rowscan(int32_t* seg, int n, int nseg, int32_t* cnt, hipStream_t s) {
    hipLaunchKernelGGL(seq_above_rowscan_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, seg, n, nseg, cnt);
    return launched("seq_above_rowscan_kernel launch");
}

// the workspace of a range selection: seg [n][ceil(M / 64)] i32 | cnt [n] i32
static size_t seq_seg_bytes(int n, int M) { return a256((size_t)n * ((M + 63) / 64) * 4); }

size_t seq_above_ws_bytes(int n, int M) {
    if (n <= 0 || M <= 0) return 0;
    return seq_seg_bytes(n, M) + a256((size_t)n * 4);
}

// fills a.nseg and a.rg, then: pass(1), the row scan, the scan, and unless the capacity is 0 (count only) pass(2)
template <class A, class Pass>
static int run_range(A& a, const Eligible& e, float thr, const RangeOut& o, hipStream_t s, Pass&& pass) {
    const int n = a.R - a.ctx;
    a.nseg = (a.M + 63) / 64;
    a.rg.row_self = e.row_self;
    a.rg.row0 = e.row0;
    a.rg.window = e.window;
    a.rg.causal = e.causal;
    a.rg.thr = thr;
    a.rg.seg = static_cast<int32_t*>(o.ws);
    int32_t* cnt = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(o.ws) + seq_seg_bytes(n, a.M));
    a.rg.row_ptr = o.row_ptr;
    a.rg.rout0 = o.rout0;
    a.rg.rows = o.rows;
    a.rg.cols = o.cols;
    a.rg.vals = o.vals;
    a.rg.codes = o.codes;
    a.rg.cap = o.cap;
    a.rg.status = o.status;
    int rc = pass(std::integral_constant<int, 1>{});
    if (rc != SGPR_OK) return rc;
    rc = launch_seq_above_rowscan(a.rg.seg, n, a.nseg, cnt, s);
    if (rc != SGPR_OK) return rc;
    rc = launch_above_scan(cnt, n, o.row_ptr, o.count, o.accumulate, s);
    if (rc != SGPR_OK || o.cap == 0) return rc;
    return pass(std::integral_constant<int, 2>{});
}

int launch_seq_above(const ScoreBlock& b, const SeqSpec& seq, const Eligible& e, float thr, const RangeOut& out,
                     hipStream_t s) {
    if (b.R - seq.ctx <= 0 || b.M <= 0) return SGPR_OK;
    SeqAboveArgs a;
    Grid g;
    const int rc = fill_tile(a, b, seq, seq.L - 1, "sequence range selection", &g);
    if (rc != SGPR_OK) return rc;
    a.fwd = (seq.dirs & SGPR_SEQ_FORWARD) ? 1 : 0;
    a.rev = (seq.dirs & SGPR_SEQ_REVERSE) ? 1 : 0;
    fill_rcp(a.rcp);
    return run_range(a, e, thr, out, s, [&](auto P) {
        return launch_tile<seq_above_kernel<decltype(P)::value>>(
            a, g, SGPR_SEQ_MAX_LEN - 1, "sequence range selection",
            decltype(P)::value == 1 ? "seq_above_kernel launch (pass 1)" : "seq_above_kernel launch (pass 2)", s);
    });
}

// arguments already checked (launch_session_filter's and launch_seq_above's, seq.min_terms in 1..L)
int launch_session_above(const ScoreBlock& b, const SeqSpec& seq, const Eligible& e, float thr, const RangeOut& out,
                         hipStream_t s) {
    if (b.R - seq.ctx <= 0 || b.M <= 0) return SGPR_OK;
    SessionAboveArgs a;
    Grid g;
    fill_paths(a, seq);
    const int rc = fill_tile(a, b, seq, a.H, "session range selection", &g);
    if (rc != SGPR_OK) return rc;
    fill_sessions(a, seq, b.R, b.M);
    a.min_terms = seq.min_terms;
    return run_range(a, e, thr, out, s, [&](auto P) {
        return by_direction(seq.dirs, [&](auto F, auto V) {
            return launch_tile<session_above_kernel<decltype(F)::value, decltype(V)::value, decltype(P)::value>>(
                a, g, SGPR_SEQ_PATH_MAX_OFFSET, "session range selection",
                decltype(P)::value == 1 ? "session_above_kernel launch (pass 1)" : "session_above_kernel launch (pass 2)",
                s);
        });
    });
}

int launch_seq_dirs(const int32_t* idx, int n, int k, const unsigned char* dir, int64_t ld, int fixed,
                    unsigned char* out, hipStream_t s) {
    const int64_t total = (int64_t)n * k;
    if (total <= 0) return SGPR_OK;
    hipLaunchKernelGGL(seq_dirs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, idx, total, k, dir, ld,
                       fixed, out);
    return launched("seq_dirs_kernel launch");
}

}  // namespace sgpr

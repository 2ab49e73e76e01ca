// Multi-session maps (sgpr_session_filter, sgpr_score_session_topk): sgpr_seq_path_filter's path-set mean where the rows
// and the columns are several trajectories stacked in time order, and sums and the window stop at the seams.  DESIGN.md §22.
//
// A session table is starts[0..n-1], starts[0] = 0, non-decreasing (a repeated value is an empty session), every value
// <= R (rows) or <= M (columns).  sess(x) = the largest j with starts[j] <= x (x < 0: session 0); lo(x) = starts[sess(x)],
// hi(x) = starts[sess(x) + 1] - 1, or the last index for the last session.  For path p and sigma = +1 forward, -1 reverse:
//
//   D_p(r, c)    = { d in 0..L-1 : r - d >= lo_row(r) and lo_col(c) <= c - sigma off_p[d] <= hi_col(c) }     a prefix
//   Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|]         fp32 additions in ascending d
//
// folded over the candidates as sgpr_seq_path_filter folds them.  With window >= 0 the end point (r, c) is EXCLUDED iff
// sess_col(c) == sess_col(self_r) and |c - self_r| <= window (self_r = row_self[r] or row0 + r): -inf, code 0.  Terms
// are never masked.
//
// session_kernel is seq_path_kernel (sgpr_seq_path.hip) with three changes: a lane's room is the distance to its own
// session's edges (c - lo, hi - c: looked up once per tile from the column table, a wave-uniform array in the kernel
// arguments), a row's depth is the distance to its session's start (the row table, walked once per tile: rows ascend),
// and the store applies the window.  Tile, halo, staging, the offsets as scalar words and the two side-by-side folds are
// that kernel's; a word read past a lane's room is still inside the tile's row (o <= H) and is dropped by the select.
#include <algorithm>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int SESS_TR = 32;     // output rows per tile
constexpr int SESS_TC = 256;    // columns per tile = threads per workgroup
constexpr int SESS_WORDS = SGPR_SEQ_MAX_LEN / 4;   // a path's offsets, four bytes to a word

struct SessionArgs {
    const float* score;   // [R][ld]
    int R, M;
    int64_t ld;
    int ctx, L;
    int n_paths, H;       // H = the largest offset of the call
    float* out;           // [R - ctx][ldo]
    int64_t ldo;
    unsigned char* code;  // [R - ctx][ldc] or nullptr
    int64_t ldc;
    const int32_t* row_self;   // [R] or nullptr: row0 + r
    int row0, window;
    int tiles_x;
    int n_row, n_col;     // sessions (>= 1)
    float rcp[SGPR_SEQ_MAX_LEN + 1];   // rcp[n] = (float)(1.0 / n), rounded once from double on the host
    uint32_t off[SGPR_SEQ_MAX_PATHS][SESS_WORDS];   // byte d of path p: off_p[d]
    int32_t row_starts[SGPR_SESSION_MAX];
    int32_t col_starts[SGPR_SESSION_MAX];
};
static_assert(sizeof(SessionArgs) < 4096, "the kernel arguments stay under 4 KB");

template <bool FWD, bool REV>
__global__ __launch_bounds__(SESS_TC) void session_kernel(const SessionArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float sess_tile[];
    __shared__ float sess_rcp[SGPR_SEQ_MAX_LEN + 1];
    const int tid = threadIdx.x, h = a.L - 1, H = a.H;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int r_base = a.ctx + ty * SESS_TR, c_base = tx * SESS_TC;
    const int rows = min(SESS_TR, a.R - r_base);         // output rows of this tile (>= 1 by the grid)
    const int pitch = SESS_TC + 2 * H;
    if (tid <= SGPR_SEQ_MAX_LEN) sess_rcp[tid] = a.rcp[tid];
    // LDS row lr holds input row r_base - h + lr, LDS column lc input column c_base - H + lc
    for (int lr = 0; lr < rows + h; ++lr) {
        const int r = r_base - h + lr;                   // < R by construction
        const float* sp = a.score + (int64_t)(r < 0 ? 0 : r) * a.ld;
        for (int lc = tid; lc < pitch; lc += SESS_TC) {
            const int c = c_base - H + lc;
            sess_tile[lr * pitch + lc] = (r >= 0 && c >= 0 && c < a.M) ? sp[c] : 0.f;
        }
    }
    __syncthreads();
    const int c = c_base + tid;
    if (c >= a.M) return;
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
    int jr = 0;                                          // the row session of the tile's current row (uniform)
    for (int i = 0; i < rows; ++i) {
        const int r = r_base + i;
        while (jr + 1 < a.n_row && a.row_starts[jr + 1] <= r) ++jr;
        const float* t0 = sess_tile + (i + h) * pitch + H + tid;
        const int nr = min(a.L, r - a.row_starts[jr] + 1);
        const float s0 = t0[0];
        float bf = 0.f, br = 0.f;
        int cf = 0, cr = 1;
        for (int p = 0; p < a.n_paths; ++p) {
            uint32_t w[SESS_WORDS];                      // the path's offsets: wave-uniform, indexed by constants below
#pragma unroll
            for (int j = 0; j < SESS_WORDS; ++j) w[j] = a.off[p][j];
            float sf = s0, sr = s0;
            int nf = 1, nb = 1;
#pragma unroll
            for (int d = 1; d < SGPR_SEQ_MAX_LEN; ++d) {
                if (d >= nr) break;                      // (uniform)
                const int o = (int)((w[d >> 2] >> (8 * (d & 3))) & 0xffu);
                const float* t = t0 - d * pitch;
                if (FWD) {
                    const float v = t[-o];
                    const bool in = o <= room_f;
                    sf = in ? sf + v : sf;
                    nf += in ? 1 : 0;
                }
                if (REV) {
                    const float v = t[o];
                    const bool in = o <= room_r;
                    sr = in ? sr + v : sr;
                    nb += in ? 1 : 0;
                }
            }
            if (FWD) {
                const float q = sf * sess_rcp[nf];
                if (p == 0 || q > bf || bf != bf) {
                    bf = q;
                    cf = p << 1;
                }
            }
            if (REV) {
                const float q = sr * sess_rcp[nb];
                if (p == 0 || q > br || br != br) {
                    br = q;
                    cr = (p << 1) | 1;
                }
            }
        }
        const bool take_rev = REV && (!FWD || br > bf || bf != bf);
        float q = take_rev ? br : bf;
        int cd = take_rev ? cr : cf;
        if (a.window >= 0) {                             // (uniform) the session window, on the end point alone
            const int self = a.row_self ? __builtin_amdgcn_readfirstlane(a.row_self[r]) : a.row0 + r;
            int ss = 0;
            for (int j = 1; j < a.n_col; ++j) ss = a.col_starts[j] <= self ? j : ss;   // (self < 0: session 0)
            const int64_t dist = (int64_t)c - (int64_t)self;
            if (ss == sc && (dist < 0 ? -dist : dist) <= (int64_t)a.window) {
                q = -__builtin_inff();
                cd = 0;
            }
        }
        const int64_t o = (int64_t)(r - a.ctx);
        a.out[o * a.ldo + c] = q;
        if (a.code) a.code[o * a.ldc + c] = (unsigned char)cd;
    }
}

template <bool FWD, bool REV>
static int launch_session(const SessionArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
    static LdsLimitOnce once;
    const int lds_max = (SESS_TR + SGPR_SEQ_MAX_LEN - 1) * (SESS_TC + 2 * SGPR_SEQ_PATH_MAX_OFFSET) * (int)sizeof(float);
    const int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(session_kernel<FWD, REV>), lds_max,
                                   "session filter");
    if (rc != SGPR_OK) return rc;
    hipLaunchKernelGGL((session_kernel<FWD, REV>), dim3(blocks), dim3(SESS_TC), lds, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "session_kernel launch");
}

// arguments already checked (paths as launch_seq_path_filter's, offsets == nullptr: the unit diagonal; tables: 1..64
// entries, the first 0, non-decreasing, <= R / <= M, or nullptr: one session)
int launch_session_filter(const float* score, int R, int M, int64_t ld, int ctx, int L, int flags, const int32_t* offsets,
                          int n_paths, const int32_t* row_starts, int n_row, const int32_t* col_starts, int n_col,
                          const int32_t* row_self, int row0, int window, float* out, int64_t ldo, unsigned char* code,
                          int64_t ldc, hipStream_t s) {
    if (R - ctx <= 0 || M <= 0) return SGPR_OK;
    SessionArgs a;
    a.score = score;
    a.R = R;
    a.M = M;
    a.ld = ld;
    a.ctx = ctx;
    a.L = L;
    a.n_paths = offsets ? n_paths : 1;
    a.H = 0;
    for (int p = 0; p < SGPR_SEQ_MAX_PATHS; ++p) {
        for (int j = 0; j < SESS_WORDS; ++j) a.off[p][j] = 0u;
        for (int d = 0; p < a.n_paths && d < L; ++d) {
            const int o = offsets ? offsets[(size_t)p * L + d] : d;
            a.off[p][d >> 2] |= (uint32_t)o << (8 * (d & 3));
            a.H = std::max(a.H, o);
        }
    }
    a.out = out;
    a.ldo = ldo;
    a.code = code;
    a.ldc = ldc;
    a.row_self = row_self;
    a.row0 = row0;
    a.window = window;
    a.n_row = row_starts ? n_row : 1;
    a.n_col = col_starts ? n_col : 1;
    for (int j = 0; j < SGPR_SESSION_MAX; ++j) {
        a.row_starts[j] = row_starts && j < n_row ? row_starts[j] : (j == 0 ? 0 : R);
        a.col_starts[j] = col_starts && j < n_col ? col_starts[j] : (j == 0 ? 0 : M);
    }
    a.rcp[0] = 0.f;
    for (int n = 1; n <= SGPR_SEQ_MAX_LEN; ++n) a.rcp[n] = (float)(1.0 / n);
    const int64_t tx = (M + SESS_TC - 1) / SESS_TC, ty = (R - ctx + SESS_TR - 1) / SESS_TR;
    if (tx * ty > 0x7fffffffLL) {
        set_error("session filter: more than 2^31 tiles");
        return SGPR_E_INVALID;
    }
    a.tiles_x = (int)tx;
    const int rows = std::min(SESS_TR, R - ctx);
    const size_t lds = (size_t)(rows + L - 1) * (SESS_TC + 2 * a.H) * sizeof(float);
    const bool fwd = (flags & SGPR_SEQ_FORWARD) != 0, rev = (flags & SGPR_SEQ_REVERSE) != 0;
    if (fwd && rev) return launch_session<true, true>(a, (unsigned)(tx * ty), lds, s);
    return fwd ? launch_session<true, false>(a, (unsigned)(tx * ty), lds, s)
               : launch_session<false, true>(a, (unsigned)(tx * ty), lds, s);
}

}  // namespace sgpr

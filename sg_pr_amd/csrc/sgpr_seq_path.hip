// Speed-tolerant sequence matching (sgpr_seq_path_filter, sgpr_score_path_topk): the mean of the scores along a PATH of
// the similarity matrix that ends in (r, c), maximised over a small set of paths.  DESIGN.md §21.
//
// A path is off[0..L-1], off[0] = 0, non-decreasing, off[L-1] <= SGPR_SEQ_PATH_MAX_OFFSET: the column distance walked
// back after d row steps (off[d] = d is sgpr_seq_filter's diagonal).  For path p and sigma = +1 forward, -1 reverse:
//
//   D_p(r, c)    = { d in 0..L-1 : r - d >= 0 and 0 <= c - sigma off_p[d] < M }     a prefix: off is monotone
//   Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|]         fp32 additions in ascending d
//
// The output is a fold over the candidates, forward paths 0..P-1 and then reverse paths 0..P-1: best starts as the first
// candidate, a later x replaces it iff x > best or best is NaN; code = direction bit | path << 1 of the winner.
//
// seq_path_kernel: seq_filter_kernel's tile (SEQP_TR output rows x SEQP_TC columns, one thread per column, lanes along
// the row when staging) with a halo of H = the call's largest offset on either side: LDS (rows + L-1) x (SEQP_TC + 2 H)
// floats, 96 768 bytes at L = 32, H = 64.  At step d lane i reads word (row - d) * pitch + i -+ off_p[d]: adjacent
// lanes, adjacent words, for every path (no bank conflict).  The offsets travel in the kernel arguments as bytes; a path's
// 32 bytes are fetched as eight wave-uniform words (scalar loads) and the d loop is unrolled, so every offset is a field
// of a scalar register.  Each lane's terms are its own prefix (off_p[d] <= c forward, <= M - 1 - c reverse): a step past
// it changes neither the sum nor the count - no term is ever replaced by a zero.  rcp[] sits in 33 words of static LDS.
#include <algorithm>

#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int SEQP_TR = 32;     // output rows per tile
constexpr int SEQP_TC = 256;    // columns per tile = threads per workgroup
constexpr int SEQP_WORDS = SGPR_SEQ_MAX_LEN / 4;   // a path's offsets, four bytes to a word

struct SeqPathArgs {
    const float* score;   // [R][ld]
    int R, M;
    int64_t ld;
    int ctx, L;
    int n_paths, H;       // H = the largest offset of the call
    float* out;           // [R - ctx][ldo]
    int64_t ldo;
    unsigned char* code;  // [R - ctx][ldc] or nullptr
    int64_t ldc;
    int tiles_x;
    float rcp[SGPR_SEQ_MAX_LEN + 1];   // rcp[n] = (float)(1.0 / n), rounded once from double on the host
    uint32_t off[SGPR_SEQ_MAX_PATHS][SEQP_WORDS];   // byte d of path p: off_p[d]
};

// FWD / REV: the directions asked for (at least one).  The two folds run side by side - forward over the paths, reverse
// over the paths - and are joined at the end; that is the fold over "forward paths, then reverse paths": a NaN forward
// best is replaced by the reverse best (the first reverse candidate replaces it, the rest fold as they do alone), any
// other forward best is replaced iff the reverse best is larger, and the reverse best is the first of its largest
// candidates either way.
template <bool FWD, bool REV>
__global__ __launch_bounds__(SEQP_TC) void seq_path_kernel(const SeqPathArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float seqp_tile[];
    __shared__ float seqp_rcp[SGPR_SEQ_MAX_LEN + 1];
    const int tid = threadIdx.x, h = a.L - 1, H = a.H;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int r_base = a.ctx + ty * SEQP_TR, c_base = tx * SEQP_TC;
    const int rows = min(SEQP_TR, a.R - r_base);         // output rows of this tile (>= 1 by the grid)
    const int pitch = SEQP_TC + 2 * H;
    if (tid <= SGPR_SEQ_MAX_LEN) seqp_rcp[tid] = a.rcp[tid];
    // LDS row lr holds input row r_base - h + lr, LDS column lc input column c_base - H + lc
    for (int lr = 0; lr < rows + h; ++lr) {
        const int r = r_base - h + lr;                   // < R by construction
        const float* sp = a.score + (int64_t)(r < 0 ? 0 : r) * a.ld;
        for (int lc = tid; lc < pitch; lc += SEQP_TC) {
            const int c = c_base - H + lc;
            seqp_tile[lr * pitch + lc] = (r >= 0 && c >= 0 && c < a.M) ? sp[c] : 0.f;
        }
    }
    __syncthreads();
    const int c = c_base + tid;
    if (c >= a.M) return;
    const int room_f = c, room_r = a.M - 1 - c;          // the largest offset a forward / reverse term may take
    for (int i = 0; i < rows; ++i) {
        const int r = r_base + i;
        const float* t0 = seqp_tile + (i + h) * pitch + H + tid;
        const int nr = min(a.L, r + 1);
        const float s0 = t0[0];
        float bf = 0.f, br = 0.f;
        int cf = 0, cr = 1;
        for (int p = 0; p < a.n_paths; ++p) {
            uint32_t w[SEQP_WORDS];                      // the path's offsets: wave-uniform, indexed by constants below
#pragma unroll
            for (int j = 0; j < SEQP_WORDS; ++j) w[j] = a.off[p][j];
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
                const float q = sf * seqp_rcp[nf];
                if (p == 0 || q > bf || bf != bf) {
                    bf = q;
                    cf = p << 1;
                }
            }
            if (REV) {
                const float q = sr * seqp_rcp[nb];
                if (p == 0 || q > br || br != br) {
                    br = q;
                    cr = (p << 1) | 1;
                }
            }
        }
        const bool take_rev = REV && (!FWD || br > bf || bf != bf);
        const int64_t o = (int64_t)(r - a.ctx);
        a.out[o * a.ldo + c] = take_rev ? br : bf;
        if (a.code) a.code[o * a.ldc + c] = (unsigned char)(take_rev ? cr : cf);
    }
}

template <bool FWD, bool REV>
static int launch_seq_path(const SeqPathArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
    static LdsLimitOnce once;
    const int lds_max = (SEQP_TR + SGPR_SEQ_MAX_LEN - 1) * (SEQP_TC + 2 * SGPR_SEQ_PATH_MAX_OFFSET) * (int)sizeof(float);
    const int rc = raise_lds_limit(&once, reinterpret_cast<const void*>(seq_path_kernel<FWD, REV>), lds_max,
                                   "sequence path filter");
    if (rc != SGPR_OK) return rc;
    hipLaunchKernelGGL((seq_path_kernel<FWD, REV>), dim3(blocks), dim3(SEQP_TC), lds, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, "seq_path_kernel launch");
}

// arguments already checked (paths: off[p][0] = 0, non-decreasing, <= SGPR_SEQ_PATH_MAX_OFFSET; 1 <= n_paths <= 16)
int launch_seq_path_filter(const float* score, int R, int M, int64_t ld, int ctx, int L, int flags, const int32_t* offsets,
                           int n_paths, float* out, int64_t ldo, unsigned char* code, int64_t ldc, hipStream_t s) {
    if (R - ctx <= 0 || M <= 0) return SGPR_OK;
    SeqPathArgs a;
    a.score = score;
    a.R = R;
    a.M = M;
    a.ld = ld;
    a.ctx = ctx;
    a.L = L;
    a.n_paths = n_paths;
    a.H = 0;
    for (int p = 0; p < SGPR_SEQ_MAX_PATHS; ++p) {
        for (int j = 0; j < SEQP_WORDS; ++j) a.off[p][j] = 0u;
        for (int d = 0; p < n_paths && d < L; ++d) {
            const int o = offsets[(size_t)p * L + d];
            a.off[p][d >> 2] |= (uint32_t)o << (8 * (d & 3));
            a.H = std::max(a.H, o);
        }
    }
    a.out = out;
    a.ldo = ldo;
    a.code = code;
    a.ldc = ldc;
    a.rcp[0] = 0.f;
    for (int n = 1; n <= SGPR_SEQ_MAX_LEN; ++n) a.rcp[n] = (float)(1.0 / n);
    const int64_t tx = (M + SEQP_TC - 1) / SEQP_TC, ty = (R - ctx + SEQP_TR - 1) / SEQP_TR;
    if (tx * ty > 0x7fffffffLL) {
        set_error("sequence path filter: more than 2^31 tiles");
        return SGPR_E_INVALID;
    }
    a.tiles_x = (int)tx;
    const int rows = std::min(SEQP_TR, R - ctx);
    const size_t lds = (size_t)(rows + L - 1) * (SEQP_TC + 2 * a.H) * sizeof(float);
    const bool fwd = (flags & SGPR_SEQ_FORWARD) != 0, rev = (flags & SGPR_SEQ_REVERSE) != 0;
    if (fwd && rev) return launch_seq_path<true, true>(a, (unsigned)(tx * ty), lds, s);
    return fwd ? launch_seq_path<true, false>(a, (unsigned)(tx * ty), lds, s)
               : launch_seq_path<false, true>(a, (unsigned)(tx * ty), lds, s);
}

}  // namespace sgpr

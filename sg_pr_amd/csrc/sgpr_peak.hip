// Distinct-place loop closures (sgpr_peak_filter, sgpr_score_peak_topk): per-row score peaks within a scan radius.
// DESIGN.md §20.
//
// A column QUALIFIES for row r iff it is eligible (sgpr_score_topk's rule: window, SGPR_TOPK_CAUSAL, self_r) and its value
// is neither NaN nor -inf (+inf qualifies) - the rule of the selection (sgpr_select.hip).  Qualifying
// columns are ordered as that selection lists them: value descending by IEEE comparison (-0.0 ties +0.0), then column
// ascending.  For a radius rho:
//
//   column c is a PEAK of row r iff it qualifies and it comes first, in that order, among the qualifying columns c'
//   with |c' - c| <= rho.
//
// - Two peaks of a row are more than rho columns apart.
// - The best qualifying column of a row is always a peak.
// - rho = 0 makes every qualifying column a peak.
// - A column that does not qualify (ineligible, NaN, -inf) neither is a peak nor suppresses anything.
// - On a plateau of equal values longer than rho only its first column is a peak: the definition is "first in its
//   neighbourhood", not "not beaten by a peak".
// - Each row is independent of every other row; nothing depends on an evaluation order (no greedy loop, no atomics).
//
// peak_filter_kernel: P[r, c] = X[r, c] (the stored bits) at a peak, -inf elsewhere; out of place.  One workgroup owns
// a strip of PEAK_STRIP columns of one row.  It stages PEAK_STRIP + 2 rho order-preserving 32-bit keys into LDS - lanes
// along the row, every global load a contiguous run; key 0 for a column that does not qualify or lies outside [0, M),
// both zeros on one key; the eligibility test happens here, once - and keeps the values of its own PEAK_STRIP / 256
// columns per thread in registers.  Sliding maxima by log-step doubling: after j = floor(log2 rho) passes
// T[i] = max(key[i .. i + 2^j - 1]) (ping-pong between two more LDS arrays, one barrier per pass, adjacent lanes on
// adjacent words in both operands: no bank conflict), and a window of rho keys is the max of two T entries:
//   leftmax(i)  = max(T[i - rho], T[i - 2^j])              keys i - rho .. i - 1
//   rightmax(i) = max(T[i + 1],   T[i + rho - 2^j + 1])    keys i + 1 .. i + rho
// c is a peak iff key > 0, leftmax < key and rightmax <= key: an equal key to the left wins (lower column first), an equal
// key to the right loses; the column index never enters a comparison.  Plain vector stores, no atomics, no scratch.
// LDS: 3 (PEAK_STRIP + 2 rho) words, 36 864 bytes at rho = 1024 - below 64 KB, no limit to raise.
#include "sgpr_internal.hpp"

namespace sgpr {

constexpr int PEAK_NT = 256;                 // threads per workgroup
constexpr int PEAK_PER = 4;                  // own columns per thread
constexpr int PEAK_STRIP = PEAK_NT * PEAK_PER;   // columns per strip (sgpr.h: SGPR_PEAK_STRIP)
static_assert(PEAK_STRIP == SGPR_PEAK_STRIP, "sgpr.h documents the strip width");

struct PeakArgs {
    const float* score;        // [n][ld]
    int n, M;
    int64_t ld;
    const int32_t* row_self;   // [n] or nullptr: row0 + r
    int row0, window, causal;
    int rho, steps;            // steps = floor(log2 rho) (0 for rho <= 1)
    float* out;                // [n][ldo]
    int64_t ldo;
    int strips;                // ceil(M / PEAK_STRIP)
};

// order-preserving image of a value that qualifies (> 0: the smallest, -FLT_MAX, maps to 0x00800000); -0.0 as +0.0
__device__ __forceinline__ unsigned peak_key(float x, bool eligible) {
    unsigned u = __float_as_uint(x);
    if (!eligible || x != x || u == 0xff800000u) return 0u;
    if (u == 0x80000000u) u = 0u;
    return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}

__global__ __launch_bounds__(PEAK_NT) void peak_filter_kernel(const PeakArgs a) {
    extern __shared__ unsigned peak_lds[];
    const int tid = threadIdx.x, rho = a.rho;
    const int r = (int)(blockIdx.x / (unsigned)a.strips), c_base = (int)(blockIdx.x % (unsigned)a.strips) * PEAK_STRIP;
    const int n = PEAK_STRIP + 2 * rho;      // LDS word i holds column c_base - rho + i
    unsigned* key = peak_lds;
    const float* sp = a.score + (int64_t)r * a.ld;
    const long long self = a.row_self ? (long long)a.row_self[r] : a.row0 + (long long)r;
    int ea, eb;
    tk_bounds(self, a.window, a.causal, ea, eb);
    // the strip's own columns: value in a register, key to LDS
    float v[PEAK_PER];
#pragma unroll
    for (int j = 0; j < PEAK_PER; ++j) {
        const int c = c_base + j * PEAK_NT + tid;
        const bool in = c < a.M;
        v[j] = in ? sp[c] : 0.f;
        key[rho + j * PEAK_NT + tid] = peak_key(v[j], in && (c < ea || c > eb));
    }
    // the halos: rho columns on either side
    for (int i = tid; i < 2 * rho; i += PEAK_NT) {
        const int li = i < rho ? i : i + PEAK_STRIP;
        const int c = c_base - rho + li;
        const bool in = c >= 0 && c < a.M;
        const float x = in ? sp[c] : 0.f;
        key[li] = peak_key(x, in && (c < ea || c > eb));
    }
    __syncthreads();
    // T_{s+1}[i] = max(T_s[i], T_s[i + 2^s]); T_0 = key, the others alternate between two more arrays
    const unsigned* T = key;
    for (int s = 0; s < a.steps; ++s) {
        unsigned* dst = peak_lds + ((s & 1) ? 2 : 1) * n;
        const int w = 1 << s;
        for (int i = tid; i < n; i += PEAK_NT) {
            const unsigned x = T[i];
            dst[i] = i + w < n ? max(x, T[i + w]) : x;   // (entries within 2^(s+1) - 1 of the end are never used)
        }
        __syncthreads();
        T = dst;
    }
    const int w = 1 << a.steps;
    float* op = a.out + (int64_t)r * a.ldo;
#pragma unroll
    for (int j = 0; j < PEAK_PER; ++j) {
        const int c = c_base + j * PEAK_NT + tid;
        if (c >= a.M) continue;
        const int i = rho + j * PEAK_NT + tid;
        const unsigned k = key[i];
        bool peak = k > 0u;
        if (rho > 0) {
            const unsigned lm = max(T[i - rho], T[i - w]);
            const unsigned rm = max(T[i + 1], T[i + rho - w + 1]);
            peak = peak && lm < k && rm <= k;
        }
        op[c] = peak ? v[j] : -INFINITY;
    }
}

// arguments already checked (0 <= rho <= SGPR_PEAK_MAX_RADIUS, ld, ldo >= M)
int launch_peak_filter(const ScoreBlock& b, const Eligible& el, int rho, float* out, int64_t ldo, hipStream_t s) {
    const int n = b.R, M = b.M;
    if (n <= 0 || M <= 0) return SGPR_OK;
    PeakArgs a;
    a.score = b.score;
    a.n = n;
    a.M = M;
    a.ld = b.ld;
    a.row_self = el.row_self;
    a.row0 = el.row0;
    a.window = el.window;
    a.causal = el.causal;
    a.rho = rho;
    a.steps = 0;
    while ((2 << a.steps) <= rho) ++a.steps;
    a.out = out;
    a.ldo = ldo;
    a.strips = (M + PEAK_STRIP - 1) / PEAK_STRIP;
    const int64_t blocks = (int64_t)n * a.strips;
    if (blocks > 0x7fffffffLL) {
        set_error("peak filter: more than 2^31 strips");
        return SGPR_E_INVALID;
    }
    const int arrays = a.steps == 0 ? 1 : (a.steps == 1 ? 2 : 3);
    const size_t lds = (size_t)arrays * (PEAK_STRIP + 2 * rho) * sizeof(unsigned);
    hipLaunchKernelGGL(peak_filter_kernel, dim3((unsigned)blocks), dim3(PEAK_NT), lds, s, a);
    return launched("peak_filter_kernel launch");
}

}  // namespace sgpr

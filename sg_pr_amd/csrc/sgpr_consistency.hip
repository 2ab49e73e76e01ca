// Pairwise-consistent loop closures (sgpr_closure_consistency, sgpr_consistent_set; include/sgpr.h):
// which verified closures agree with one another through the odometry of the drives, and a large set that agrees pair
// by pair.
//
//   cc_prep_kernel    one thread per closure: the void test, G = (C o T) o R^-1, H = T^-1 o C^-1 and R into the workspace
//   cc_pair_kernel    one workgroup per CC_ROWS rows of the bit matrix; a wave owns the 64 columns of one word, keeps
//                     their G / H / R in registers and walks the workgroup's rows, one ballot word per row; the row
//                     degrees are the popcounts of those ballots, summed per wave and then over the four waves in LDS
//   cs_clique_kernel  one workgroup per group: the candidate set is a bit row in LDS; the counts popcount(row_v & cand)
//                     of the candidates are kept up to date from what leaves cand (64-bit words, a power-of-two team of
//                     lanes per row) and every round takes the maximum of the key (count, -index) - a maximum of
//                     distinct integers, the same in any order
//
// Every float64 operation of the definition is rounded on its own (contraction is off for the whole file; sqrt is the
// correctly rounded one), so the bit matrix is reproducible bit for bit (tests/consistency_ref.py).  Plain vector
// stores only; no atomics on global memory.
#include "sgpr_internal.hpp"
#include "sgpr_map.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int CC_T = 256;        // threads of the prep and pair kernels
constexpr int CC_ROWS = 8;       // rows of the bit matrix per workgroup of the pair kernel
constexpr int CS_T = 1024;       // threads of the clique kernel
constexpr int CS_WAVES = CS_T / 64;

// the workspace of sgpr_closure_consistency: members i32 [C] first (what the header promises), then G, H, R f64 [C][4]
struct CcWs {
    int32_t* members;
    double *G, *H, *R;
};

__host__ __device__ inline size_t cc_members_bytes(int C) { return ((size_t)C * 4 + 255) / 256 * 256; }

CcWs cc_carve(void* ws, int C) {
    CcWs w;
    char* b = static_cast<char*>(ws);
    w.members = reinterpret_cast<int32_t*>(b);
    w.G = reinterpret_cast<double*>(b + cc_members_bytes(C));
    w.H = w.G + (size_t)C * 4;
    w.R = w.H + (size_t)C * 4;
    return w;
}

__global__ __launch_bounds__(CC_T) void cc_prep_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                       const double* __restrict__ T, int C, const double* __restrict__ Xr,
                                                       int MR, const double* __restrict__ Xc, int MC,
                                                       const int32_t* __restrict__ group, int n_groups, CcWs w) {
    const int p = blockIdx.x * CC_T + threadIdx.x;
    if (p >= C) return;
    const int r = rows[p], c = cols[p], g = group[p];
    bool ok = r >= 0 && r < MR && c >= 0 && c < MC && g >= 0 && g < n_groups;
    Se2 t = se2_load(T + (size_t)p * 4), rp = {1.0, 0.0, 0.0, 0.0}, cp = rp;
    if (ok) {
        rp = se2_load(Xr + (size_t)r * 4);
        cp = se2_load(Xc + (size_t)c * 4);
    }
    ok = ok && se2_finite(t) && se2_finite(rp) && se2_finite(cp);
    if (!ok) t = rp = cp = Se2{1.0, 0.0, 0.0, 0.0};      // a void closure is never read back; keep its slots defined
    se2_store(w.G + (size_t)p * 4, se2_compose(se2_compose(cp, t), se2_inverse(rp)));
    se2_store(w.H + (size_t)p * 4, se2_compose(se2_inverse(t), se2_inverse(cp)));
    se2_store(w.R + (size_t)p * 4, rp);
    w.members[p] = ok ? g : -1;
}

// the test on (a, b), a < b, from G_a, R_a, H_b, R_b
__device__ __forceinline__ bool cc_test(const Se2& Ga, const Se2& Ra, const Se2& Hb, const Se2& Rb, double max_trans,
                                        double min_cos, double lever_gain) {
    const Se2 D = se2_compose(se2_compose(Hb, Ga), Rb);
    const double dx = Rb.x - Ra.x, dy = Rb.y - Ra.y;
    const double lever = sqrt(dx * dx + dy * dy);
    const double tau = max_trans + lever_gain * lever;
    return D.c >= min_cos && D.x * D.x + D.y * D.y <= tau * tau;
}

__global__ __launch_bounds__(CC_T) void cc_pair_kernel(CcWs w, int C, int W, double max_trans, double min_cos,
                                                       double lever_gain, unsigned long long* __restrict__ adj,
                                                       int32_t* __restrict__ degree) {
    __shared__ int deg[CC_T / 64][CC_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = blockIdx.x * CC_ROWS;
    const int nrow = min(CC_ROWS, C - p0);
    int mydeg[CC_ROWS];
#pragma unroll
    for (int r = 0; r < CC_ROWS; ++r) mydeg[r] = 0;
    for (int word = wave; word < W; word += CC_T / 64) {
        const int q = word * 64 + lane;
        const bool qin = q < C;
        const size_t qs = (size_t)(qin ? q : 0) * 4;
        const int gq = qin ? w.members[qs / 4] : -1;
        const Se2 Gq = se2_load(w.G + qs), Hq = se2_load(w.H + qs), Rq = se2_load(w.R + qs);
        unsigned long long mine = 0ull;
#pragma unroll
        for (int r = 0; r < CC_ROWS; ++r) {
            if (r < nrow) {                    // (uniform)
                const int p = p0 + r;
                const int gp = w.members[p];
                const Se2 Gp = se2_load(w.G + (size_t)p * 4), Hp = se2_load(w.H + (size_t)p * 4),
                          Rp = se2_load(w.R + (size_t)p * 4);
                const bool up = p < q;         // the test is the one on (min, max): the matrix is symmetric by construction
                const bool bit = gq >= 0 && gq == gp && q != p &&
                                 cc_test(up ? Gp : Gq, up ? Rp : Rq, up ? Hq : Hp, up ? Rq : Rp, max_trans, min_cos, lever_gain);
                const unsigned long long bal = __ballot(bit);
                mydeg[r] += __popcll(bal);
                if (lane == r) mine = bal;
            }
        }
        if (lane < nrow) adj[(size_t)(p0 + lane) * W + word] = mine;
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < CC_ROWS; ++r) deg[wave][r] = mydeg[r];
    }
    __syncthreads();
    if ((int)threadIdx.x < nrow) {
        int d = 0;
        for (int v = 0; v < CC_T / 64; ++v) d += deg[v][threadIdx.x];
        degree[p0 + threadIdx.x] = d;
    }
}

// One workgroup per group g.  ws: the members of every group, ascending, group after group (int32 [C]); this workgroup
// writes only its own segment, which starts at the number of closures in groups below g.
__global__ __launch_bounds__(CS_T) void cs_clique_kernel(const unsigned long long* __restrict__ adj, int C, int W,
                                                         const int32_t* __restrict__ group, int n_groups,
                                                         int32_t* __restrict__ rank, int32_t* __restrict__ group_size,
                                                         int32_t* __restrict__ ws) {
    __shared__ unsigned long long cand[SGPR_CONSISTENCY_MAX_CLOSURES / 64];
    __shared__ unsigned short lrank[SGPR_CONSISTENCY_MAX_CLOSURES];
    __shared__ unsigned long long rem[SGPR_CONSISTENCY_MAX_CLOSURES / 64];
    __shared__ unsigned short nzw[SGPR_CONSISTENCY_MAX_CLOSURES / 64];
    __shared__ unsigned long long wkey[CS_WAVES];
    __shared__ int wcnt[2][CS_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < W; i += CS_T) cand[i] = 0ull;
    for (int i = tid; i < C; i += CS_T) lrank[i] = 0xffffu;
    __syncthreads();

    // members of g in ascending order into ws[below ..), and the candidate bits
    int below = 0, n = 0;      // `below` is per thread until reduced; n is uniform
    for (int base = 0; base < C; base += CS_T) {
        const int p = base + tid;
        const int gp = p < C ? group[p] : -1;
        const bool valid = gp >= 0 && gp < n_groups;
        if (valid && gp < g) ++below;
        if (blockIdx.x == 0 && p < C && !valid) rank[p] = -1;       // closures of no group: written here, once
        const bool mem = gp == g;
        const unsigned long long bal = __ballot(mem);
        if (lane == 0) {
            wcnt[0][wave] = __popcll(bal);
            cand[(base >> 6) + wave] = bal;     // word of this wave's 64 closures ((base + 64 wave) / 64 < W when any is < C)
        }
        __syncthreads();
        int pre = 0, tot = 0;
        for (int v = 0; v < CS_WAVES; ++v) {
            const int c = wcnt[0][v];
            pre += v < wave ? c : 0;
            tot += c;
        }
        // (the segment start is not known yet: park the in-group position in lrank, the list is written below)
        if (mem) lrank[p] = (unsigned short)(n + pre + __popcll(bal & ((1ull << lane) - 1ull)));
        n += tot;
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off);
    if (lane == 0) wcnt[1][wave] = below;
    __syncthreads();
    below = 0;
    for (int v = 0; v < CS_WAVES; ++v) below += wcnt[1][v];
    int32_t* list = ws + below;
    for (int p = tid; p < C; p += CS_T) {
        const unsigned short pos = lrank[p];
        if (pos != 0xffffu) {
            list[pos] = p;
            lrank[p] = 0xffffu;
        }
    }
    __syncthreads();      // (the list is read back by other threads of this workgroup)

    // The counts d(v) = popcount(row_v & cand & ~bit v) are kept, not recounted: when cand loses the set `rem`, d(v) of
    // a closure that stays falls by popcount(row_v & rem) - the same integers at a cost of (candidates x non-zero words
    // of rem) per round.  lrank[v] holds d(v) while v is a candidate, its rank once chosen, 0xffff once dropped.
    // The first pass is the same step from d = 0 with rem = cand.
    for (int word = tid; word < W; word += CS_T) rem[word] = cand[word];
    __syncthreads();
    int chosen = 0, vs = -1;
    for (int round = 0; round <= n; ++round) {
        // the words of rem that hold a bit, ascending (W <= 256: one word per thread of the first four waves)
        const bool has = tid < W && rem[tid] != 0ull;
        const unsigned long long hb = __ballot(has);
        if (lane == 0 && wave < 4) wcnt[0][wave] = __popcll(hb);
        __syncthreads();
        int nz = 0, pre = 0;
        for (int v = 0; v < 4; ++v) {
            pre += v < wave ? wcnt[0][v] : 0;
            nz += wcnt[0][v];
        }
        if (has) nzw[pre + __popcll(hb & ((1ull << lane) - 1ull))] = (unsigned short)tid;
        __syncthreads();
        // a team of lanes per member: the smallest power of two that covers the nz words, at most a wave
        int lpr = 1;
        while (lpr < nz && lpr < 64) lpr <<= 1;
        const int per_wave = 64 / lpr, sub = lane / lpr, sl = lane % lpr;
        for (int i = wave * per_wave + sub; i < n; i += CS_WAVES * per_wave) {
            const int v = list[i];
            const unsigned long long bit = 1ull << (v & 63);
            if (rem[v >> 6] & bit) {                        // leaves (round 0: nobody - cand and rem are the same set)
                if (round > 0 && sl == 0) lrank[v] = v == vs ? (unsigned short)(chosen - 1) : (unsigned short)0xffffu;
                if (round > 0) continue;
            } else if (!(cand[v >> 6] & bit)) {
                continue;                                   // left in an earlier round
            }
            const unsigned long long* row = adj + (size_t)v * W;
            int c = 0;
            for (int j = sl; j < nz; j += lpr) {
                const int word = nzw[j];
                unsigned long long m = row[word] & rem[word];
                if (word == (v >> 6)) m &= ~bit;            // (matters in round 0 only: later v is not in rem)
                c += __popcll(m);
            }
            for (int off = lpr >> 1; off > 0; off >>= 1) c += __shfl_xor(c, off);
            if (sl == 0) lrank[v] = round == 0 ? (unsigned short)c : (unsigned short)(lrank[v] - c);
        }
        __syncthreads();
        // the maximum of the key (count << 32 | ~index) over the candidates; 0 = none (an index is below 2^14)
        unsigned long long best = 0ull;
        for (int i = tid; i < n; i += CS_T) {
            const int v = list[i];
            if ((cand[v >> 6] >> (v & 63)) & 1ull) {
                const unsigned long long key = ((unsigned long long)lrank[v] << 32) | (unsigned)~(unsigned)v;
                best = key > best ? key : best;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        if (lane == 0) wkey[wave] = best;
        __syncthreads();
        best = 0ull;
        for (int v = 0; v < CS_WAVES; ++v) best = wkey[v] > best ? wkey[v] : best;
        if (best == 0ull) break;            // (uniform: cand is empty)
        vs = (int)~(unsigned)(best & 0xffffffffull);
        ++chosen;
        const unsigned long long* row = adj + (size_t)vs * W;
        for (int word = tid; word < W; word += CS_T) {
            const unsigned long long old = cand[word];
            unsigned long long m = old & row[word];
            if (word == (vs >> 6)) m &= ~(1ull << (vs & 63));
            cand[word] = m;
            rem[word] = old & ~m;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < n; i += CS_T) {
        const int p = list[i];
        const unsigned short r = lrank[p];
        rank[p] = r == 0xffffu ? -1 : (int)r;
    }
    if (tid == 0) group_size[g] = chosen;
}

}  // namespace

size_t closure_consistency_ws_bytes(int C) { return C <= 0 ? 0 : cc_members_bytes(C) + (size_t)C * 12 * sizeof(double); }

size_t consistent_set_ws_bytes(int C) { return C <= 0 ? 0 : cc_members_bytes(C); }

int launch_closure_consistency(const int32_t* rows, const int32_t* cols, const double* T, int C, const double* Xr, int MR,
                               const double* Xc, int MC, const int32_t* group, int n_groups, double max_trans,
                               double min_cos, double lever_gain, unsigned long long* adj, int32_t* degree, void* ws,
                               hipStream_t s) {
    const CcWs w = cc_carve(ws, C);
    const int W = (C + 63) / 64;
    hipLaunchKernelGGL(cc_prep_kernel, dim3((C + CC_T - 1) / CC_T), dim3(CC_T), 0, s, rows, cols, T, C, Xr, MR, Xc, MC,
                       group, n_groups, w);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "cc_prep_kernel launch");
    hipLaunchKernelGGL(cc_pair_kernel, dim3((C + CC_ROWS - 1) / CC_ROWS), dim3(CC_T), 0, s, w, C, W, max_trans, min_cos,
                       lever_gain, adj, degree);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "cc_pair_kernel launch");
    return SGPR_OK;
}

int launch_consistent_set(const unsigned long long* adj, int C, const int32_t* group, int n_groups, int32_t* rank,
                          int32_t* group_size, void* ws, hipStream_t s) {
    hipLaunchKernelGGL(cs_clique_kernel, dim3(n_groups), dim3(CS_T), 0, s, adj, C, (C + 63) / 64, group, n_groups, rank,
                       group_size, static_cast<int32_t*>(ws));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "cs_clique_kernel launch");
    return SGPR_OK;
}

}  // namespace sgpr

// What the consumers of a resident score matrix (sgpr_metrics.hip) and the fused epilogues of the all-pairs tail
// (sgpr_score.hip) both do, once: counting scores between thresholds (tree, descent, rank lookup, wave-aggregated LDS
// add, the workgroup's slab), the slab layout and its fold, and the K dispatch of the per-row lists.  Device and host
// helpers only; the one kernel of the family (the fold) lives in sgpr_metrics.hip behind launch_slab_fold.
#pragma once
#include <type_traits>

#include "sgpr_internal.hpp"

namespace sgpr {

// a negative or NaN score: its order among the thresholds is undefined, the pair is counted as skipped
__device__ __forceinline__ bool ev_bad(float s) { return __float_as_uint(s) > 0x7f800000u; }

// ------------------------------------------------------------------ the slab of one counting workgroup
// [slab_words(T)] u32: counters 0..T, padded to an even count | skipped pairs (u64) | rank sum (u64)
__host__ __device__ inline int slab_counters(int T) { return (T + 2) & ~1; }
__host__ __device__ inline int slab_words(int T) { return slab_counters(T) + 4; }
__device__ __forceinline__ unsigned long long* slab_tail(unsigned* slab, int words) {
    return reinterpret_cast<unsigned long long*>(slab + words - 4);
}
__device__ __forceinline__ const unsigned long long* slab_tail(const unsigned* slab, int words) {
    return reinterpret_cast<const unsigned long long*>(slab + words - 4);
}
// out[i] (+)= the sum over the slabs of counter i (0..T), then out[T + 1] = skipped and out[T + 2] = rank sum;
// out_t (optional): the counter sums once more, counter t * per + q at [q * 1024 + t] (sgpr_metrics.hip)
int launch_slab_fold(const unsigned* slabs, int n_slabs, int words, int T, unsigned long long* out, int accumulate,
                     unsigned long long* out_t, int per, hipStream_t stream);

// ------------------------------------------------------------------ counting scores between T ascending thresholds
// bucket b of a score s = #{q : thr[q] <= s}; with a rank table also the rank sum over the counted scores of
// 2 #{positive pairs > s} + #{positive pairs == s}: bucket b > 0 holds the values rank[(b - 1) * gpt .. b * gpt), eight
// per record, thr[b - 1] the first of them
struct ThrView {
    const float* tree;                   // [1 << thr_levels(T)] the thresholds as a search tree, LDS
    unsigned* cnt;                       // [T + 1] the workgroup's counters, LDS
    const unsigned long long* at_least;  // [T] positive pairs with a value >= thr[q] (ranking only), LDS
    const sgpr_rank_group* rank;         // [T * gpt] or nullptr
    int T, gpt;
};
// the levels of the tree: 1 << thr_levels(T) is the power of two above T
__host__ __device__ inline int thr_levels(int T) {
#ifdef __HIP_DEVICE_COMPILE__
    return T > 0 ? 32 - __clz(T) : 0;
#else
    int lg = 0;
    while ((1 << lg) <= T) ++lg;
    return lg;
#endif
}

// The thresholds as a complete binary search tree in breadth-first order (node 1 = root, children 2k / 2k + 1), padded
// with +inf: the probes of one level are neighbours in LDS.  In the sorted array the probes of the upper levels sit a
// power of two >= 32 words apart - all lanes of a wave in ONE bank, a 64-way conflict per step.
__device__ __forceinline__ void thr_build_tree(float* tree, int lg, const float* __restrict__ thr, int T, int tid,
                                               int stride) {
    for (int node = tid; node < (1 << lg); node += stride) {
        float v = INFINITY;
        if (node > 0) {
            const int l = 31 - __clz(node), i = node - (1 << l);
            const int idx = ((2 * i + 1) << (lg - 1 - l)) - 1;            // position of the node's key in sorted order
            if (idx < T) v = thr[idx];
        }
        tree[node] = v;
    }
}

// four independent branch-free descents, interleaved: right whenever the key is <= s -> the buckets of s[0..3]
__device__ __forceinline__ void thr_descend4(const ThrView& t, const float (&s)[4], int (&b)[4]) {
    const int lg = thr_levels(t.T);
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = 1;
    for (int lvl = 0; lvl < lg; ++lvl) {
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = 2 * b[q] + ((t.tree[b[q]] <= s[q]) ? 1 : 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = min(b[q] - (1 << lg), t.T);
}

// The rank terms of the counted ones among four scores.  A bucket's values (and how many pairs carry each) arrive in one
// round of independent 16-byte loads from the L2-resident table, W scores at a time (2 where the scores stream from
// memory, 1 in the register-bound tail): pairs above s = pairs from the bucket's first value on - pairs of the bucket's
// values <= s; bucket 0: s lies below every positive value, all P = at_least[0] pairs rank above it
template <int W>
__device__ __forceinline__ unsigned long long thr_rank4(const ThrView& t, const float (&s)[4], const int (&b)[4],
                                                        const bool (&counted)[4]) {
    unsigned long long rank2 = 0ull;
#pragma unroll
    for (int q0 = 0; q0 < 4; q0 += W) {
        unsigned le[W], eq[W];
#pragma unroll
        for (int e = 0; e < W; ++e) le[e] = eq[e] = 0u;
#pragma unroll W                                          // (W = 2: two rounds of records in flight, 6 % of the matrix kernel
                                                           //  with ranking; W = 1 compiles as it does without the pragma)
        for (int gi = 0; gi < t.gpt; ++gi) {
            float4 v[W][2];
            uint4 m[W][2];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const uint4* rec = reinterpret_cast<const uint4*>(t.rank + (size_t)max(b[q0 + e] - 1, 0) * t.gpt + gi);
                v[e][0] = *reinterpret_cast<const float4*>(rec);
                v[e][1] = *reinterpret_cast<const float4*>(rec + 1);
                m[e][0] = rec[2];
                m[e][1] = rec[3];
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float x = s[q0 + e];
                const float vv[8] = {v[e][0].x, v[e][0].y, v[e][0].z, v[e][0].w, v[e][1].x, v[e][1].y, v[e][1].z, v[e][1].w};
                const unsigned mm[8] = {m[e][0].x, m[e][0].y, m[e][0].z, m[e][0].w, m[e][1].x, m[e][1].y, m[e][1].z, m[e][1].w};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    le[e] += vv[i] <= x ? mm[i] : 0u;
                    eq[e] += vv[i] == x ? mm[i] : 0u;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const int bq = b[q0 + e];
            const unsigned long long gt_s = bq > 0 ? t.at_least[bq - 1] - le[e] : t.at_least[0];
            rank2 += counted[q0 + e] ? 2ull * gt_s + (bq > 0 ? eq[e] : 0u) : 0ull;
        }
    }
    return rank2;
}

// Wave-aggregated counting (called by whole waves): sigmoid scores pile up in a few buckets, and 64 lanes hitting one
// LDS counter serialise.  Up to three rounds take the bucket of the first waiting lane with ONE atomic for all the lanes
// that share it; whoever is left counts on its own.
__device__ __forceinline__ void thr_add4(unsigned* cnt, const int (&b)[4], const bool (&counted)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int idx = counted[q] ? b[q] : -1;
        unsigned long long todo = __ballot(idx >= 0);
#pragma unroll 1
        for (int round = 0; round < 3 && todo; ++round) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lidx = __shfl(idx, leader);
            const unsigned long long same = __ballot(idx == lidx);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&cnt[lidx], (unsigned)__popcll(same));
            if (idx == lidx) idx = -1;
            todo &= ~same;
            if (__popcll(same) < 4) break;               // scattered buckets: the rounds would only add instructions
        }
        if (idx >= 0) atomicAdd(&cnt[idx], 1u);
    }
}

// four scores of a lane, those with counted[q] into the counters and the rank sum (whole waves)
template <int W>
__device__ __forceinline__ void thr_count4(const ThrView& t, const float (&s)[4], const bool (&counted)[4],
                                           unsigned long long& rank2) {
    int b[4];
    thr_descend4(t, s, b);
    if (t.rank) rank2 += thr_rank4<W>(t, s, b, counted);
    thr_add4(t.cnt, b, counted);
}

// The workgroup's closing step (every thread, `threads` of them): the lanes' skipped counts and rank sums meet in
// tail[2] (LDS) and the counters and the tail go to the workgroup's own slab - no global atomic; the fold adds the slabs
__device__ __forceinline__ void thr_close(const ThrView& t, unsigned long long* tail, unsigned long long nbad,
                                          unsigned long long rank2, unsigned* __restrict__ slab, int tid, int threads) {
    if (tid < 2) tail[tid] = 0ull;
    __syncthreads();
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        rank2 += __shfl_xor(rank2, m);
        nbad += __shfl_xor(nbad, m);
    }
    if ((tid & 63) == 0) {
        if (nbad) atomicAdd(&tail[0], nbad);
        if (rank2) atomicAdd(&tail[1], rank2);
    }
    __syncthreads();
    for (int i = tid; i <= t.T; i += threads) slab[i] = t.cnt[i];
    if (tid < 2) slab_tail(slab, slab_words(t.T))[tid] = tail[tid];
}

// ------------------------------------------------------------------ the K = 1 / 4 / 8 / 16 instances of the row lists
// launches launch(std::integral_constant<int, K>()) for the compiled list instance of k (the first k of its K = 1, 4, 8 or
// 16 entries)
template <class Launch>
static int launch_list_k(int k, const char* what, Launch&& launch) {
    if (k <= 1)
        launch(std::integral_constant<int, 1>());
    else if (k <= 4)
        launch(std::integral_constant<int, 4>());
    else if (k <= 8)
        launch(std::integral_constant<int, 8>());
    else
        launch(std::integral_constant<int, 16>());
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SGPR_OK : hip_fail(e, what);
}

}  // namespace sgpr

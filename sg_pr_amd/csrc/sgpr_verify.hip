// Geometric verification of loop-closure candidates (sgpr_verify_pairs): planar consensus between the labelled 3-D
// centres of two graphs.  DESIGN.md §19.
//
//   hypothesis  h = (i, i', j, j'): two nodes of A and two same-labelled nodes of B whose planar distances agree
//               (lu >= min_base, lu lv > 0, |lu - lv| <= tau_edge) fix a rotation about z and a translation in the plane
//   inl(h)      = nodes p of A with a same-label node q of B within tau_z in height and tau_in in the plane after h
//   result      = the hypothesis with the most inliers (ties: the lowest (i, i', j, j')), one float64 least-squares step
//
// Every float32 / float64 operation of the definition is rounded on its own (contraction is off for the whole file; `/`
// and sqrtf are the correctly rounded ones), so the record is reproducible bit for bit (tests/geo_ref.py).
//
// verify_kernel: one 256-thread workgroup per pair.
//   load     thread t owns slot t of both graphs.  A is compacted in slot order (base pairs are enumerated in that
//            order), B is ranked by (label, slot): a node of A then sees its same-label nodes of B as one range.
//   enumerate  a workgroup-uniform loop over the base pairs (i, i') of A; the running hypothesis count is a uniform
//            register, so the cap is one comparison.  Per base pair the (j, j') candidates of the two ranges are length-
//            tested 256 at a time and the admissible ones appended to a ring of 1024 packed entries: positions come from a
//            ballot per wave and four per-wave counts in LDS (two sets, alternating, so one barrier per chunk suffices).
//   evaluate whenever the ring holds 256 entries every lane takes one: it keeps its own c, s, tx, ty and walks A's nodes
//            against their ranges of B - the same (p, q) sequence in every lane, so all LDS reads are broadcasts.
//   best     max-reduction over the key  inliers << 32 | ~(i << 24 | i' << 16 | j << 8 | j')  (slot indices).
//   refine   lane p finds q(p); lane 0 runs the float64 sums in ascending p; lane p recounts under the rounded result.
// No global atomics; every loop is bounded by the slot counts and the cap (a base pair adds at most nB^2 past it).
#include "sgpr_internal.hpp"

#pragma clang fp contract(off)

namespace sgpr {

constexpr int VF_T = 256;          // threads per workgroup = SGPR_VERIFY_MAX_NODES
constexpr int VF_RING = 1024;      // ring entries (< 256 left over + <= 256 appended + 256 being evaluated, with room)

struct VerifyArgs {
    const float* ca;       // [GA][N][3]
    const int32_t* la;     // [GA][N]
    const float* cb;
    const int32_t* lb;
    int GA, GB, N;
    const int32_t* ia;     // [P]
    const int32_t* ib;
    float tau_edge, tin2, tau_z, min_base;
    unsigned max_hyp;
    sgpr_verify_result* out;
};

struct VfXf {
    float c, s, tx, ty;
};

// A node: x, y, z, (range of B: start | end << 16).  B node: x, y, z, slot.
__device__ __forceinline__ VfXf vf_transform(const float4& a0, const float4& a1, const float4& b0, const float4& b1) {
    const float ux = a1.x - a0.x, uy = a1.y - a0.y;
    const float vx = b1.x - b0.x, vy = b1.y - b0.y;
    const float lu = sqrtf(ux * ux + uy * uy), lv = sqrtf(vx * vx + vy * vy);
    const float den = lu * lv;
    VfXf t;
    t.c = (ux * vx + uy * vy) / den;
    t.s = (ux * vy - uy * vx) / den;
    const float max_ = 0.5f * (a0.x + a1.x), may = 0.5f * (a0.y + a1.y);
    const float mbx = 0.5f * (b0.x + b1.x), mby = 0.5f * (b0.y + b1.y);
    t.tx = mbx - (t.c * max_ - t.s * may);
    t.ty = mby - (t.s * max_ + t.c * may);
    return t;
}

// q(p): the qualifying node of p's range with the smallest planar distance, the first of equals (slots ascend inside a
// range); -1: p is no inlier
__device__ __forceinline__ int vf_match(const float4 a, const float4* __restrict__ B, const VfXf t, float tin2, float tau_z) {
    const unsigned rg = __float_as_uint(a.w);
    const int q0 = (int)(rg & 0xffffu), q1 = (int)(rg >> 16);
    const float px = (t.c * a.x - t.s * a.y) + t.tx;
    const float py = (t.s * a.x + t.c * a.y) + t.ty;
    int bq = -1;
    float bd = 0.f;
    for (int q = q0; q < q1; ++q) {
        const float4 b = B[q];
        const float dx = px - b.x, dy = py - b.y;
        const float d2 = dx * dx + dy * dy;
        if (fabsf(a.z - b.z) <= tau_z && d2 <= tin2 && (bq < 0 || d2 < bd)) {
            bq = q;
            bd = d2;
        }
    }
    return bq;
}

__device__ __forceinline__ void vf_store_empty(sgpr_verify_result* o, unsigned flags, bool zeroed) {
    const float fn = zeroed ? 0.f : __uint_as_float(0x7fc00000u);
    const double dn = zeroed ? 0.0 : __longlong_as_double(0x7ff8000000000000LL);
    o->inliers = 0;
    o->inliers_refined = 0;
    for (int k = 0; k < 4; ++k) {
        o->base[k] = zeroed ? 0 : -1;
        o->coarse[k] = fn;
        o->refined[k] = dn;
    }
    o->hypotheses = 0;
    o->flags = flags;
    o->rmse = dn;
}

__global__ __launch_bounds__(VF_T) void verify_kernel(const VerifyArgs g) {
    __shared__ float4 A[VF_T];            // compacted, slot order
    __shared__ float4 B[VF_T];            // ranked by (label, slot)
    __shared__ int aslot[VF_T];
    __shared__ int rawlb[VF_T];           // B's labels by slot (ranking)
    __shared__ unsigned ring[VF_RING];
    __shared__ int wcnt[2][4];
    __shared__ unsigned long long wkey[4];
    __shared__ int match[VF_T];
    __shared__ int misc[8];               // 0 non-finite flag, 1 winning entry, 2..5 refined inlier counts per wave
    __shared__ float rxf[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = g.N;
    sgpr_verify_result* o = g.out + blockIdx.x;
    const int ga = g.ia[blockIdx.x], gb = g.ib[blockIdx.x];
    if (ga < 0 || ga >= g.GA || gb < 0 || gb >= g.GB) {       // (uniform)
        if (tid == 0) vf_store_empty(o, SGPR_VERIFY_INVALID_INDEX, true);
        return;
    }

    // ---- load: thread t owns slot t of both graphs
    float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
    int la = -1, lb = -1;
    if (tid < N) {
        const size_t sa = (size_t)ga * N + tid, sb = (size_t)gb * N + tid;
        la = g.la[sa];
        lb = g.lb[sb];
        ax = g.ca[sa * 3];
        ay = g.ca[sa * 3 + 1];
        az = g.ca[sa * 3 + 2];
        bx = g.cb[sb * 3];
        by = g.cb[sb * 3 + 1];
        bz = g.cb[sb * 3 + 2];
    }
    const bool ra = la >= 0, rb = lb >= 0;
    const float big = 3.4028234663852886e38f;
    const bool bad = (ra && !(fabsf(ax) <= big && fabsf(ay) <= big && fabsf(az) <= big)) ||
                     (rb && !(fabsf(bx) <= big && fabsf(by) <= big && fabsf(bz) <= big));
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long balA = __ballot(ra);
    rawlb[tid] = rb ? lb : -1;
    if (tid == 0) misc[0] = 0;
    if (lane == 0) wcnt[0][wave] = __popcll(balA);
    __syncthreads();
    if (bad) misc[0] = 1;
    int nA = 0, posA = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = wcnt[0][w];
        if (w < wave) posA += c;
        nA += c;
    }
    posA += __popcll(balA & below);
    // rank of this thread's B node among B's real nodes by (label, slot); this thread's A node's range of that order
    int rankB = 0, lo = 0, eq = 0, nB = 0;
    for (int t = 0; t < N; ++t) {
        const int l = rawlb[t];
        if (l < 0) continue;
        ++nB;
        rankB += (l < lb || (l == lb && t < tid)) ? 1 : 0;
        lo += l < la ? 1 : 0;
        eq += l == la ? 1 : 0;
    }
    if (ra) {
        A[posA] = make_float4(ax, ay, az, __uint_as_float((unsigned)lo | ((unsigned)(lo + eq) << 16)));
        aslot[posA] = tid;
    }
    if (rb) B[rankB] = make_float4(bx, by, bz, __int_as_float(tid));
    __syncthreads();
    if (misc[0]) {                                              // (uniform)
        if (tid == 0) vf_store_empty(o, SGPR_VERIFY_NONFINITE, false);
        return;
    }

    // ---- enumerate and evaluate
    unsigned tail = 0, head = 0;          // appended / evaluated entries so far (uniform); tail = hypotheses
    unsigned long long best = 0ull;       // this lane's best key (0: none)
    unsigned best_e = 0u;
    int par = 1;                          // wcnt set of the next chunk (set 0 was used by the load)
    bool truncated = false;

    auto evaluate = [&](unsigned e) {
        const int i0 = (int)(e & 255u), i1 = (int)((e >> 8) & 255u), j0 = (int)((e >> 16) & 255u), j1 = (int)(e >> 24);
        const float4 b0 = B[j0], b1 = B[j1];
        const VfXf t = vf_transform(A[i0], A[i1], b0, b1);
        unsigned inl = 0;
        for (int p = 0; p < nA; ++p) {
            const float4 a = A[p];
            const unsigned rg = __float_as_uint(a.w);
            const int q0 = (int)(rg & 0xffffu), q1 = (int)(rg >> 16);
            const float px = (t.c * a.x - t.s * a.y) + t.tx;
            const float py = (t.s * a.x + t.c * a.y) + t.ty;
            bool hit = false;
            for (int q = q0; q < q1; ++q) {
                const float4 b = B[q];
                const float dx = px - b.x, dy = py - b.y;
                hit = hit || (fabsf(a.z - b.z) <= g.tau_z && dx * dx + dy * dy <= g.tin2);
            }
            inl += hit ? 1u : 0u;
        }
        const unsigned slots = ((unsigned)aslot[i0] << 24) | ((unsigned)aslot[i1] << 16) |
                               ((unsigned)__float_as_int(b0.w) << 8) | (unsigned)__float_as_int(b1.w);
        const unsigned long long key = ((unsigned long long)inl << 32) | (unsigned long long)(~slots);
        if (key > best) {
            best = key;
            best_e = e;
        }
    };

    for (int i0 = 0; i0 < nA && !truncated; ++i0) {
        const float4 a0 = A[i0];
        const unsigned rg0 = __float_as_uint(a0.w);
        const int s1 = (int)(rg0 & 0xffffu), n1 = (int)(rg0 >> 16) - s1;
        for (int i1 = i0 + 1; i1 < nA; ++i1) {
            if (tail >= g.max_hyp) {
                truncated = true;
                break;
            }
            const float4 a1 = A[i1];
            const unsigned rg1 = __float_as_uint(a1.w);
            const int s2 = (int)(rg1 & 0xffffu), n2 = (int)(rg1 >> 16) - s2;
            const float ux = a1.x - a0.x, uy = a1.y - a0.y;
            const float lu = sqrtf(ux * ux + uy * uy);
            const int total = n1 * n2;
            if (!(lu >= g.min_base) || total == 0) continue;
            for (int c0 = 0; c0 < total; c0 += VF_T) {
                const int cand = c0 + tid;
                bool adm = false;
                int j0 = 0, j1 = 0;
                if (cand < total) {
                    j0 = s1 + cand / n2;
                    j1 = s2 + cand % n2;
                    const float4 b0 = B[j0], b1 = B[j1];
                    const float vx = b1.x - b0.x, vy = b1.y - b0.y;
                    const float lv = sqrtf(vx * vx + vy * vy);
                    // (den = lu lv > 0: no zero length, no underflowing product - c and s are never 0 / 0)
                    adm = j0 != j1 && lu * lv > 0.f && fabsf(lu - lv) <= g.tau_edge;
                }
                const unsigned long long bal = __ballot(adm);
                if (lane == 0) wcnt[par][wave] = __popcll(bal);
                int pos = __popcll(bal & below);
                // (the position needs the other waves' counts: the entry is written after the barrier, into a slot no
                //  lane reads before the next barrier)
                __syncthreads();
                int added = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int c = wcnt[par][w];
                    if (w < wave) pos += c;
                    added += c;
                }
                if (adm)
                    ring[(tail + (unsigned)pos) & (VF_RING - 1)] =
                        (unsigned)i0 | ((unsigned)i1 << 8) | ((unsigned)j0 << 16) | ((unsigned)j1 << 24);
                tail += (unsigned)added;
                par ^= 1;
                if (tail - head >= (unsigned)VF_T) {
                    __syncthreads();                            // the entries of this chunk are in the ring
                    evaluate(ring[(head + (unsigned)tid) & (VF_RING - 1)]);
                    head += VF_T;
                }
            }
        }
    }
    __syncthreads();
    if (head + (unsigned)tid < tail) evaluate(ring[(head + (unsigned)tid) & (VF_RING - 1)]);

    if (tail == 0u) {                                           // (uniform)
        if (tid == 0) vf_store_empty(o, SGPR_VERIFY_NO_HYPOTHESIS, false);
        return;
    }

    // ---- the best hypothesis of the workgroup
    unsigned long long wbest = best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(wbest, off);
        wbest = other > wbest ? other : wbest;
    }
    if (lane == 0) wkey[wave] = wbest;
    __syncthreads();
    unsigned long long kbest = wkey[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) kbest = wkey[w] > kbest ? wkey[w] : kbest;
    if (best == kbest) misc[1] = (int)best_e;                    // (keys of distinct hypotheses differ: one lane)
    __syncthreads();
    const unsigned e = (unsigned)misc[1];
    const int i0 = (int)(e & 255u), i1 = (int)((e >> 8) & 255u), j0 = (int)((e >> 16) & 255u), j1 = (int)(e >> 24);
    const VfXf t = vf_transform(A[i0], A[i1], B[j0], B[j1]);

    // ---- refinement: lane p finds q(p), lane 0 sums in ascending p
    if (tid < nA) match[tid] = vf_match(A[tid], B, t, g.tin2, g.tau_z);
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        double sax = 0.0, say = 0.0, sbx = 0.0, sby = 0.0;
        for (int p = 0; p < nA; ++p) {
            const int q = match[p];
            if (q < 0) continue;
            ++n;
            sax = sax + (double)A[p].x;
            say = say + (double)A[p].y;
            sbx = sbx + (double)B[q].x;
            sby = sby + (double)B[q].y;
        }
        double rc = (double)t.c, rs = (double)t.s, rtx = (double)t.tx, rty = (double)t.ty;
        if (n >= 2) {
            const double dn = (double)n;
            const double cax = sax / dn, cay = say / dn, cbx = sbx / dn, cby = sby / dn;
            double D = 0.0, X = 0.0;
            for (int p = 0; p < nA; ++p) {
                const int q = match[p];
                if (q < 0) continue;
                const double xa = (double)A[p].x - cax, ya = (double)A[p].y - cay;
                const double xb = (double)B[q].x - cbx, yb = (double)B[q].y - cby;
                D = D + (xa * xb + ya * yb);
                X = X + (xa * yb - ya * xb);
            }
            const double nrm = sqrt(D * D + X * X);
            if (nrm != 0.0) {
                rc = D / nrm;
                rs = X / nrm;
                rtx = cbx - (rc * cax - rs * cay);
                rty = cby - (rs * cax + rc * cay);
            }
        }
        double rmse = __longlong_as_double(0x7ff8000000000000LL);
        if (n > 0) {
            double ssq = 0.0;
            for (int p = 0; p < nA; ++p) {
                const int q = match[p];
                if (q < 0) continue;
                const double x = (double)A[p].x, y = (double)A[p].y;
                const double dx = ((rc * x - rs * y) + rtx) - (double)B[q].x;
                const double dy = ((rs * x + rc * y) + rty) - (double)B[q].y;
                ssq = ssq + (dx * dx + dy * dy);
            }
            rmse = sqrt(ssq / (double)n);
        }
        o->inliers = (int32_t)(kbest >> 32);
        o->base[0] = aslot[i0];
        o->base[1] = aslot[i1];
        o->base[2] = __float_as_int(B[j0].w);
        o->base[3] = __float_as_int(B[j1].w);
        o->hypotheses = tail;
        o->flags = truncated ? SGPR_VERIFY_TRUNCATED : 0u;
        o->coarse[0] = t.c;
        o->coarse[1] = t.s;
        o->coarse[2] = t.tx;
        o->coarse[3] = t.ty;
        o->refined[0] = rc;
        o->refined[1] = rs;
        o->refined[2] = rtx;
        o->refined[3] = rty;
        o->rmse = rmse;
        rxf[0] = (float)rc;
        rxf[1] = (float)rs;
        rxf[2] = (float)rtx;
        rxf[3] = (float)rty;
    }
    __syncthreads();
    VfXf r;
    r.c = rxf[0];
    r.s = rxf[1];
    r.tx = rxf[2];
    r.ty = rxf[3];
    const bool in2 = tid < nA && vf_match(A[tid], B, r, g.tin2, g.tau_z) >= 0;
    const unsigned long long bal2 = __ballot(in2);
    if (lane == 0) misc[2 + wave] = __popcll(bal2);
    __syncthreads();
    if (tid == 0) o->inliers_refined = misc[2] + misc[3] + misc[4] + misc[5];
}

int launch_verify_pairs(const float* ca, const int32_t* la, int GA, const float* cb, const int32_t* lb, int GB, int N,
                        const int32_t* ia, const int32_t* ib, int64_t P, float tau_edge, float tau_in, float tau_z,
                        float min_base, int max_hyp, sgpr_verify_result* out, hipStream_t s) {
    VerifyArgs a;
    a.ca = ca;
    a.la = la;
    a.cb = cb;
    a.lb = lb;
    a.GA = GA;
    a.GB = GB;
    a.N = N;
    a.tau_edge = tau_edge;
    a.tin2 = tau_in * tau_in;      // the product is formed once, in float32
    a.tau_z = tau_z;
    a.min_base = min_base;
    a.max_hyp = (unsigned)max_hyp;
    const int64_t step = 1 << 30;  // pairs per launch (a grid dimension holds fewer than 2^31 workgroups)
    for (int64_t p0 = 0; p0 < P; p0 += step) {
        const int64_t n = P - p0 < step ? P - p0 : step;
        a.ia = ia + p0;
        a.ib = ib + p0;
        a.out = out + p0;
        hipLaunchKernelGGL(verify_kernel, dim3((unsigned)n), dim3(VF_T), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "verify_kernel launch");
    }
    return SGPR_OK;
}

}  // namespace sgpr

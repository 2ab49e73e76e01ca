// The building blocks the map back end shares: planar poses, the lock-free union-find, the
// open-addressing cell table, the cells of the map frame, the session rule, workspace carving and the host-side checks
// of a session table and of the arguments the entry points have in common.  One definition of each; sgpr_cluster /
// consistency / localize / posegraph / score / api include it, and the landmark files through sgpr_map_grid.hpp, which
// adds what only they share (the cell grid, the linking step, the numbering of roots, the planar fit).
//
// Floating-point contraction: a header included above a file's `#pragma clang fp contract(off)` is not covered by it,
// and files without that line include this one too.  Every function here that multiplies and adds carries the pragma
// in its own body, so its products are rounded on their own wherever it is inlined.
#pragma once
#include <initializer_list>

#include "sgpr_internal.hpp"

namespace sgpr {

// ------------------------------------------------------------------ planar poses (c, s, x, y), float64
struct Se2 {
    double c, s, x, y;
};

__device__ __forceinline__ Se2 se2_compose(const Se2& a, const Se2& b) {
#pragma clang fp contract(off)
    Se2 r;
    r.c = a.c * b.c - a.s * b.s;
    r.s = a.s * b.c + a.c * b.s;
    r.x = (a.c * b.x - a.s * b.y) + a.x;
    r.y = (a.s * b.x + a.c * b.y) + a.y;
    return r;
}

__device__ __forceinline__ Se2 se2_inverse(const Se2& a) {
#pragma clang fp contract(off)
    Se2 r;
    r.c = a.c;
    r.s = -a.s;
    r.x = -(a.c * a.x + a.s * a.y);
    r.y = a.s * a.x - a.c * a.y;
    return r;
}

__device__ __forceinline__ Se2 se2_load(const double* p) {
    const double2 lo = *reinterpret_cast<const double2*>(p), hi = *reinterpret_cast<const double2*>(p + 2);
    return Se2{lo.x, lo.y, hi.x, hi.y};
}

__device__ __forceinline__ void se2_store(double* p, const Se2& v) {
    *reinterpret_cast<double2*>(p) = make_double2(v.c, v.s);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v.x, v.y);
}

__device__ __forceinline__ bool se2_finite(const Se2& v) {
    return isfinite(v.c) && isfinite(v.s) && isfinite(v.x) && isfinite(v.y);
}

// ------------------------------------------------------------------ sessions
// sess(k) = the largest j with starts[j] <= k (starts[0] = 0, non-decreasing, a repeated value is an empty session;
// k < 0: session 0).  Uniform trip count, a select per step.  The table is the array in the kernel's arguments.
__device__ __forceinline__ int session_of(const int32_t* starts, int n, int k) {
    int s = 0;
    for (int j = 1; j < n; ++j) s = starts[j] <= k ? j : s;
    return s;
}

// ------------------------------------------------------------------ the open-addressing table (64-bit keys)
// SIZING.  A table has table_slots(n) >= 2 n slots for at most n distinct keys, so it is never more than half full:
// insertion and lookup always reach their key or an empty slot.  Lookups run in a later kernel than the insertions.
// I is the slot index type (the callers' tables are indexed by `unsigned` or `unsigned long long`).
constexpr unsigned long long TABLE_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}
// slot of `key`, inserting it when absent
template <class I>
__device__ __forceinline__ I table_insert(unsigned long long* keys, I mask, unsigned long long key) {
    I s = (I)mix64(key) & mask;
    while (true) {
        const unsigned long long old = atomicCAS(&keys[s], TABLE_EMPTY, key);
        if (old == TABLE_EMPTY || old == key) return s;
        s = (s + 1) & mask;
    }
}
// slot of `key`, or (I)TABLE_EMPTY when absent (the table is complete: built by an earlier kernel)
template <class I>
__device__ __forceinline__ I table_find(const unsigned long long* keys, I mask, unsigned long long key) {
    I s = (I)mix64(key) & mask;
    while (true) {
        const unsigned long long k = keys[s];
        if (k == key) return s;
        if (k == TABLE_EMPTY) return (I)TABLE_EMPTY;
        s = (s + 1) & mask;
    }
}

// ------------------------------------------------------------------ cells of the map frame (the landmark files)
// Cell width of a label: a hair wider than its radius, and never below LM_MIN_CELL.
//
// Two points in range are never two cells apart.  Let a >= b be one coordinate of two points that link, w the width.
// The rule gives fl(dx dx) <= fl(r r) up to the roundings of the products and the sum, i.e. |dx| <= r (1 + 2^-50), and
// dx = fl(a - b), so a - b <= r (1 + 2^-49).  w >= r 1.001 (1 - 2^-52), so (a - b) / w < 1 - 9e-4.  Both quotients are
// rounded: |a|, |b| <= 2^37 and w >= 0.5 bound them by 2^38 and each rounding error by 2^-53 2^38 = 2^-15, together
// 6.2e-5.  So fl(a / w) - fl(b / w) < 1, and floor() of two numbers less than 1 apart differs by at most 1 (division
// by a positive w is monotone, so the difference is not negative either).  |quotient| <= 2^38 fits a long long.
// A width above the radius only adds candidates; the pair test is the caller's, exact.  r = +inf: w = inf, every
// quotient is +-0, one cell.  (One product, one quotient: nothing here can contract; the pragma keeps it so.)
constexpr double LM_MIN_CELL = 0.5;

__device__ __forceinline__ double lm_cell_width(double r) {
#pragma clang fp contract(off)
    return fmax(r * 1.001, LM_MIN_CELL);
}
__device__ __forceinline__ long long lm_cell_coord(double v, double w) {
#pragma clang fp contract(off)
    return (long long)floor(v / w);
}

// The key is a HASH of (label, ix, iy), not a packing: 2 x 39 bits of cell coordinate and 6 of label do not fit.  Two
// cells with one key share a list; why that never costs an answer is argued where the lists are walked (grid_near,
// sgpr_map_grid.hpp).
__device__ __forceinline__ unsigned long long lm_cell_key(int label, long long ix, long long iy) {
    unsigned long long k = mix64((unsigned long long)ix + 0x9e3779b97f4a7c15ull * (unsigned long long)(label + 1));
    k = mix64(k ^ ((unsigned long long)iy * 0xd6e8feb86659fd93ull));
    return k == TABLE_EMPTY ? 0ull : k;
}

// ------------------------------------------------------------------ the lock-free lowest-root union-find
// parent[x] = x initially; uf_unite always hooks the LARGER root under the smaller, so a component's root is its
// lowest index whatever the execution order.
//
// VISIBILITY.  Per-XCD L2s are not coherent with one another and a CU's L1 is never refreshed by other CUs' stores.
// The forest is rewritten by other CUs while it is read, so it is read and written with agent-scope relaxed atomics
// (served past L1 / L2 where the agent's coherence point is) and hooked with a device-scope CAS.  Once the uniting
// kernel has ended the forest is final, and uf_root_final walks it with the same loads.
//
// TERMINATION.  Path halving only ever replaces a pointer by an ancestor, and a root's parent only ever decreases, so
// uf_find ends.  The only loop that depends on another workgroup is uf_unite's CAS retry, and a failed CAS means that
// another thread's CAS succeeded (lock-free: some thread always makes progress).  Nothing waits on a flag, a counter or
// a lock.
__device__ __forceinline__ int ld_parent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_parent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(int* parent, int x) {
    int p = ld_parent(parent + x);
    while (p != x) {                       // path halving
        const int gp = ld_parent(parent + p);
        if (gp != p) st_parent(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;      // hook the larger root under the smaller
    }
}
// the root of x in a final forest (no store: the flatten kernels record it themselves)
__device__ __forceinline__ int uf_root_final(const int* parent, int x) {
    while (true) {
        const int up = ld_parent(parent + x);
        if (up == x) return x;
        x = up;
    }
}

// ------------------------------------------------------------------ host: workspace carving
inline size_t align256(size_t v) { return a256(v); }   // (the map back end's name for it)

// slots of a table for n keys: a power of two, at least 1024 and at least 2 n (SIZING above)
inline size_t table_slots(size_t n) {
    size_t h = 1024;
    while (h < 2 * n) h <<= 1;
    return h;
}

// consecutive arrays of a workspace, each starting 256-byte aligned from the base
struct Carver {
    unsigned char* p;
    template <class T>
    T* take(size_t count) {
        T* r = reinterpret_cast<T*>(p);
        p += align256(count * sizeof(T));
        return r;
    }
};

// ------------------------------------------------------------------ host: session tables (the rules of sgpr.h)
// `which` names the table in the message ("row", "column") or is empty.  false: the message is set
inline bool session_table_ok(const char* fn, const char* which, const int32_t* starts, int n, int limit) {
    const std::string head = std::string(fn) + ": ", w = *which ? std::string(which) + " " : std::string();
    if (n < 0 || n > SGPR_SESSION_MAX) {
        set_error(head + "the number of " + w + "sessions must lie in 0.." + std::to_string(SGPR_SESSION_MAX));
        return false;
    }
    if (!starts || n == 0) {
        if (!starts && n == 0) return true;               // one session
        set_error(head + (starts ? "a " : "NULL ") + w + "session table with n = " + std::to_string(n));
        return false;
    }
    if (starts[0] != 0) {
        set_error(head + "the " + w + "session table does not start at 0");
        return false;
    }
    for (int j = 1; j < n; ++j)
        if (starts[j] < starts[j - 1]) {
            set_error(head + "the " + w + "session table has a decreasing entry at " + std::to_string(j));
            return false;
        }
    if (starts[n - 1] > limit) {
        set_error(head + "the " + w + "session table has an entry past " + std::to_string(limit));
        return false;
    }
    return true;
}

// a checked table into a kernel's arguments; none means one session that starts at 0
inline void fill_session_table(int32_t* dst, int* n_dst, const int32_t* h_starts, int n_sessions) {
    *n_dst = n_sessions > 0 ? n_sessions : 1;
    for (int s = 0; s < *n_dst; ++s) dst[s] = n_sessions > 0 ? h_starts[s] : 0;
}

// ------------------------------------------------------------------ host: the argument checks of the landmark entry points
// false: the message is set.  The words are what the host tests match; the return code and the order of an entry
// point's checks stay its own.
struct NamedInt {
    const char* name;
    int v;
};
// the first negative of the list: "<name> <v> is negative"
inline bool no_negative(const std::string& fn, std::initializer_list<NamedInt> values) {
    for (const NamedInt& s : values)
        if (s.v < 0) {
            set_error(fn + ": " + s.name + " " + std::to_string(s.v) + " is negative");
            return false;
        }
    return true;
}
// v >= 0, so not NaN either
inline bool not_negative(const std::string& fn, const char* name, double v) {
    if (v >= 0.0) return true;
    set_error(fn + ": " + name + " is negative or NaN");
    return false;
}
inline bool workspace_ok(const std::string& fn, size_t have, size_t need) {
    if (have >= need) return true;
    set_error(fn + ": workspace of " + std::to_string(have) + " bytes, " + std::to_string(need) + " needed");
    return false;
}

}  // namespace sgpr

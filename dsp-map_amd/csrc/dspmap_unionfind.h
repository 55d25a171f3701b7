// dspmap_unionfind.h -- find / unite on a label array whose entries only ever decrease (dspmap_objects.hip; tools/objects_uf_check.cpp runs
// the same code on the host, sequentially and from threads).  Compiles for host and device: the memory comes through the template
// parameter Mem, { int load(int i); int atomic_min(int i, int v) /* returns the old value */; } -- atomicMin on the device, a
// compare-exchange loop on the host.
//
// The array L holds, for every SET cell x, L[x] <= x, and a chain x, L[x], L[L[x]], ... stays inside one connected component.  A cell
// with L[x] == x is a root.  Values are only ever lowered (atomic_min), so the invariant survives every interleaving, and a value read
// late or stale is an EARLIER value of that entry: a larger member of the same chain, from which the chase still only descends.
//
// Termination, by construction and not by the state of the memory:
//   uf_find   follows p = L[x].  p == x ends the chase; p outside [0, x) is a fault and ends it too; otherwise x becomes p < x.  x is a
//             non-negative int that strictly decreases, so the loop takes at most (start value) steps -- at most V -- whatever L holds.
//   uf_unite  takes the roots, orders them a > b and does old = atomic_min(L[a], b).  old == a: a was a root and now hangs below b, done.
//             old > a breaks the invariant: a fault, done.  Otherwise somebody linked a below old < a first; whichever of old and b is
//             now stored at L[a], the other one still has to meet it, so the round continues with (old, b).  Both are < a, their roots
//             are no larger, so the next round's a is strictly smaller: at most (first a) rounds.
// Both loops also carry an explicit trip bound n (the number of cells).  Running out of it, or meeting a broken invariant, returns a
// fault code; the caller records it (the counts buffer's fault word) and goes on.  Nothing here waits for another thread.
#pragma once

#if defined(__HIPCC__)
#define UF_HD __host__ __device__ __forceinline__
#else
#define UF_HD inline
#endif

enum { UF_OK = 0, UF_FAULT_CHAIN = 1, UF_FAULT_BOUND = 2, UF_FAULT_ORDER = 3 };

// the root of x (>= 0), or -1 with *fault set: L[x] outside [0, x] on the way, or more than n steps
template <class Mem> UF_HD int uf_find(Mem& m, int x, int n, int* fault) {
    for (int i = 0; i <= n; ++i) {
        const int p = m.load(x);
        if (p == x) return x;
        if (p < 0 || p > x) { *fault = UF_FAULT_CHAIN; return -1; }
        x = p;
    }
    *fault = UF_FAULT_BOUND;
    return -1;
}

// the components of a and b become one; UF_OK or a fault code
template <class Mem> UF_HD int uf_unite(Mem& m, int a, int b, int n) {
    int fault = UF_OK;
    for (int i = 0; i <= n; ++i) {
        a = uf_find(m, a, n, &fault);
        if (a < 0) return fault;
        b = uf_find(m, b, n, &fault);
        if (b < 0) return fault;
        if (a == b) return UF_OK;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = m.atomic_min(a, b);
        if (old == a) return UF_OK;
        if (old > a || old < 0) return UF_FAULT_ORDER;
        a = old;
    }
    return UF_FAULT_BOUND;
}

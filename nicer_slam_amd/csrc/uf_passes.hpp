// uf_passes.hpp -- the three passes of the lock-free union-find that labels mesh components (csrc/mesh_clean.hip).
// The bodies compile for the device (hipcc: atomicCAS, relaxed loads) and, unchanged, as host C++ (GCC / clang __atomic
// builtins) so that the same code can be run by many host threads in a CPU test (tests/uf_host_check.cpp).
//
// State: parent[V] int32.  Invariant: parent[x] <= x at all times, and a slot only ever decreases.  Hence every walk
// x -> parent[x] is strictly descending until it reaches a root (parent[r] == r) and ends within V steps; a root is only ever
// changed by a compare-and-swap on its own slot from r to a smaller root, so two trees are joined exactly once and never form a
// cycle; and when every union has returned, the root of a tree is the smallest vertex index in it whatever the interleaving was.
// Every loop carries a step cap as well; a cap that trips sets *status and leaves the loop (a logic error is reported, never spun on).
#pragma once
#include <cstdint>

namespace nsa {

#if defined(__HIPCC__)
#define NSA_UF_FN __device__ __forceinline__
NSA_UF_FN int32_t uf_load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
NSA_UF_FN void uf_store(int32_t* p, int32_t v) { *p = v; }
NSA_UF_FN int32_t uf_cas(int32_t* p, int32_t expect, int32_t desired) { return atomicCAS(p, expect, desired); }
#else
#define NSA_UF_FN static inline
NSA_UF_FN int32_t uf_load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
NSA_UF_FN void uf_store(int32_t* p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
NSA_UF_FN int32_t uf_cas(int32_t* p, int32_t expect, int32_t desired) {
    __atomic_compare_exchange_n(p, &expect, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;               // the value found (== the old `expect` when the swap happened)
}
#endif

constexpr uint32_t kUfCapFind = 1u, kUfCapHook = 2u;     // status bits

NSA_UF_FN bool uf_valid_face(int32_t a, int32_t b, int32_t c, uint32_t V) {
    return a >= 0 && b >= 0 && c >= 0 && (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;
}

// root of x with path halving: parent[x] is moved from p to parent[p] (<= p: the invariant holds whoever wins)
NSA_UF_FN int32_t uf_find(int32_t* parent, int32_t x, uint32_t V, uint32_t* status) {
    for (uint32_t step = 0; step <= V; ++step) {
        const int32_t p = uf_load(parent + x);
        if (p == x) return x;
        const int32_t g = uf_load(parent + p);
        if (g != p) uf_cas(parent + x, p, g);
        x = g;
    }
    *status |= kUfCapFind;
    return x;
}

// join the trees of a and b: the larger root is hooked under the smaller by a CAS on the root's own slot; a lost CAS means
// that root was hooked by someone else meanwhile (at most V - 1 hooks ever succeed), so the retry starts from the new roots
NSA_UF_FN void uf_unite(int32_t* parent, int32_t a, int32_t b, uint32_t V, uint32_t* status) {
    for (uint32_t tries = 0; tries <= V; ++tries) {
        a = uf_find(parent, a, V, status);
        b = uf_find(parent, b, V, status);
        if (a == b || *status) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (uf_cas(parent + hi, hi, lo) == hi) return;
    }
    *status |= kUfCapHook;
}

// pass 1, one call per vertex
NSA_UF_FN void uf_pass_init(int32_t* parent, int32_t* vertex_label, uint32_t v) {
    parent[v] = (int32_t)v;
    vertex_label[v] = -1;
}

// pass 2, one call per face: marks the three vertices of a valid face as referenced (vertex_label = 0, the same value from
// every face) and joins them
NSA_UF_FN void uf_pass_face(int32_t* parent, int32_t* vertex_label, const int32_t* faces, uint32_t f, uint32_t V,
                            uint32_t* status) {
    const int32_t a = faces[3ull * f], b = faces[3ull * f + 1], c = faces[3ull * f + 2];
    if (!uf_valid_face(a, b, c, V)) return;
    uf_store(vertex_label + a, 0);
    uf_store(vertex_label + b, 0);
    uf_store(vertex_label + c, 0);
    if (a != b) uf_unite(parent, a, b, V, status);
    if (b != c) uf_unite(parent, b, c, V, status);
}

// pass 3, one call per vertex, after every call of pass 2 has returned: the label (-1 for an unreferenced vertex)
NSA_UF_FN int32_t uf_pass_label(int32_t* parent, int32_t* vertex_label, uint32_t v, uint32_t V, uint32_t* status) {
    const int32_t l = vertex_label[v] < 0 ? -1 : uf_find(parent, (int32_t)v, V, status);
    vertex_label[v] = l;
    return l;
}

}  // namespace nsa

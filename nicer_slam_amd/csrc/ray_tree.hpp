// ray_tree.hpp -- the layout of the ray-cast tree (C ABI Section 17): its node record, the padded box of a face, the views
// into the caller's buffer and their order there.  Built by mesh_raycast.hip; walked by it and, for face-against-face queries, by
// mesh_intersect.hip (Section 25), which reads the boxes as supersets of the exact ones.
#pragma once
#include "octree_build.hpp"

namespace nsa {
namespace rc {

using bulk::up256;
using octree::Head;
using octree::kLeafBit;
using octree::kMaxLevel;
using octree::max_nodes;

constexpr float kPadRel = 0x1p-20f;

struct Node {                    // 32 bytes
    float lo[3], hi[3];
    uint32_t skip;               // first node behind the subtree; kLeafBit set on a leaf
    uint32_t begin;              // first sorted face
};
static_assert(sizeof(Node) == 32, "Node is read as one 32-byte record");

// the padded box of a usable face: six fp32, each rounded outwards
__device__ __forceinline__ void face_box(const float (&a)[3], const float (&b)[3], const float (&c)[3], float (&box)[6]) {
#pragma clang fp contract(off)
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) s = fmaxf(s, fmaxf(fmaxf(fabsf(a[k]), fabsf(b[k])), fabsf(c[k])));
    const float pad = s * kPadRel;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = fminf(fminf(a[k], b[k]), c[k]) - pad, hi = fmaxf(fmaxf(a[k], b[k]), c[k]) + pad;
        box[k] = nextafterf(lo, -INFINITY);
        box[3 + k] = nextafterf(hi, INFINITY);
    }
}

struct Tree {                    // views into the caller's buffer (nsa_tri_ray_workspace bytes)
    Head* head;
    uint32_t* order;             // [F]: face indices in sorted order, the usable ones first
    uint32_t* skey;              // [F]: sorted keys
    uint32_t* base;              // [F + 1]: exclusive prefix sum of h
    float* fbox;                 // [F][6]: the padded box of the face at each sorted position
    Node* node;                  // [max_nodes(F)]
    uint32_t* end;               // [max_nodes(F)]: one past the node's last sorted face
    uint32_t* child;             // [max_nodes(F)][8]: the child of each octant, 0 = none (the root is nobody's child)
    uint32_t* keys[2];           // [F] each: radix ping-pong
    uint32_t* tmp;               // [F]
    uint32_t* counts;            // [256 * 256]

    // the hooks of octree_build.hpp.  k_heads: the box of the face at sorted position i (zeros where there is no usable face)
    static __device__ __forceinline__ void sorted_face(const Tree& t, const float* __restrict__ v, uint32_t V,
                                                       const int32_t* __restrict__ f, uint32_t i, uint32_t g, bool live) {
        float box[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            float a[3], b[3], c[3];
            if (tri::load_face(v, V, f, g, a, b, c) == 0) face_box(a, b, c, box);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) t.fbox[6ull * i + k] = box[k];
    }
    // k_nodes: no children yet
    static __device__ __forceinline__ void new_node(const Tree& t, uint32_t n) {
#pragma unroll
        for (int o = 0; o < 8; ++o) t.child[8ull * n + o] = 0;
    }
};

__host__ __device__ inline uint64_t carve(void* ws, uint32_t F, Tree* out) {
    const uint64_t nmax = max_nodes(F);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    Tree t;
    t.head = reinterpret_cast<Head*>(take(sizeof(Head)));
    t.order = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.skey = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.base = reinterpret_cast<uint32_t*>(take(4ull * ((uint64_t)F + 1)));
    t.fbox = reinterpret_cast<float*>(take(24ull * F));
    t.node = reinterpret_cast<Node*>(take(sizeof(Node) * nmax));
    t.end = reinterpret_cast<uint32_t*>(take(4ull * nmax));
    t.child = reinterpret_cast<uint32_t*>(take(32ull * nmax));
    t.keys[0] = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.keys[1] = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.tmp = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    if (out) *out = t;
    return o;
}

}  // namespace rc
}  // namespace nsa

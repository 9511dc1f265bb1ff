// mesh_cc.hip -- connected components of an indexed triangle mesh on the device
// (include/sdfr.h, "Mesh connected components"; DESIGN.md "Mesh components"): label,
// measure, keep, compact.
//
// Labelling.  A lock-free union-find over the triangle edges (the ECL-CC shape: Jaiganesh
// and Burtscher, HPDC 2018).  parent lives in the caller's `label` array.
//
//   cc_init_kernel     parent[v] = v
//   cc_union_kernel    one thread per face (a, b, c): union(a, b), union(b, c)
//   cc_flatten_kernel  its own launch after the union: label[v] = root(v)
//
//   find(x)      walks parent from x to a root (parent[r] == r) and halves the path on the
//                way (parent[prev] = grandparent).
//   union(a, b)  ra = find(a), rb = find(b); while they differ: hi = max, lo = min,
//                atomicCAS(&parent[hi], hi, lo).  Success: done.  Failure: the CAS returns
//                what parent[hi] holds now; the side that was hi continues with the find of
//                that value.
//
// Termination and correctness.  Invariant: parent[x] <= x always, and parent[x] names a
// vertex of x's own tree.  init establishes it; a successful CAS writes lo < hi into a
// root; a halving store writes a value that was read further up x's own chain, so it is
// < x and in x's tree (trees only ever merge).  A vertex that stops being a root never
// becomes one again, because only the CAS writes to roots and it writes a smaller value.
// (a) A chase visits strictly decreasing indices >= 0, so it ends.  A halving store may
// replace a smaller value another thread stored a moment earlier with a larger one that is
// still below x: the chain gets longer again by a step, never cyclic.  (b) A CAS fails only
// when parent[hi] != hi, that is, another thread hooked hi under a smaller vertex; the
// value returned is < hi, so the pair (ra, rb) of a union strictly decreases in its larger
// member with every failure, and the union ends after at most hi failures.  (c) At most
// V - 1 CASes succeed in total, each removing one root for good.  No thread ever waits for
// a value another thread has yet to write: every loop makes progress on its own reads, so
// there is no lock, no inter-workgroup barrier and no dependence on scheduling.
// When union(a, b) returns, a and b are in one tree for good.  Every hook puts the larger
// root under the smaller, so a tree's root is the smallest vertex in it: after all unions
// root(v) is the smallest vertex index of v's component, whatever the interleaving, and
// `label` is a pure function of the mesh.
//
// The racy reads and the halving stores are relaxed agent-scope __hip_atomic_load / _store
// (no torn or cached-stale values across XCDs); the hook is an ordinary global atomicCAS on
// int32.  Stale reads are harmless: an old parent is still an ancestor-or-self in the tree.
//
// Index validation.  A face with an index outside [0, V) is never dereferenced: the union
// kernel (and every later kernel that reads faces) skips it and sets a device error word,
// which the host call reads back with its counts and turns into SDFR_EINVAL.
//
// Ranking.  is_root[v] = (label[v] == v), the exclusive scan of sdfr_scan.h, then
// comp[v] = rank[label[v]]: dense ids 0..C-1 in increasing order of the smallest vertex.
// A vertex no face references is a component of its own with 0 faces.
//
// Statistics (cc_stats_*).  Integer atomics only, so every number is reproducible bit for
// bit: n_vertices / n_faces by atomicAdd on uint32; bbox (over the component's vertices) by
// atomicMin / atomicMax on the order-preserving uint32 image of the float (sign bit set:
// all bits flipped, else sign bit flipped), decoded in place by a last kernel; area as
// unsigned 64-bit fixed point in units of u.
//   Unit rule.  d = the largest edge of the mesh's bounding box (fp64, from the fp32
//   extremes), x = 2 d^2 max(F, 1): no triangle inside the box exceeds 1.5 d^2 <= 2 d^2,
//   so the mesh's area is <= x.  u = 2^(k - 61) with k the exponent of frexp(x)
//   (x <= 2^k < 2 x); u = 1 when x is 0 or not finite.  Then sum(area / u) <= 2^61 and the
//   roundings add < F / 2 <= 2^29: the sum stays below 2^62.
//   Face area.  0.5 |(b - a) x (c - a)| in fp64 from the fp32 vertices (nothing contracted),
//   divided by u (exact: a power of two) and rounded to nearest (llrint; clamped to
//   [0, 2^61], 0 for a NaN).
//   Error bound.  For a component of Fc faces, |area_q u - exact area| <= Fc u / 2 from the
//   rounding, plus the fp64 evaluation: <= 16 * 2^-53 d^2 per face, and d^2 <= 2^60 u / F
//   by the unit rule, so <= 2^11 u over the whole mesh.  Together Fc u / 2 + 2^11 u.
// Marching-cubes indices are spatially coherent, so a wave nearly always holds elements of
// one component: when the component id is uniform over a wave's valid lanes the wave reduces
// with shuffles and its first valid lane issues ONE atomic per statistic; otherwise each lane
// issues its own.  (Without this a one-component 3.5 M-face mesh is 3.5 M atomics on one
// address.)  The four waves of a workgroup leave their results in LDS, and when they agree
// on the id one thread issues the atomics for all four: a quarter of the atomics again.  All
// forms add the same integers, so the result does not depend on which ran.  The mesh's own
// box is the union of the components' boxes (one thread per component, reduced per wave).
//
// Selection and compaction (the sdfr_mc_count / sdfr_mc_emit pattern).  count: a face is
// kept when its indices are valid and keep[comp[a]]; a vertex when keep[comp[v]] -- with
// drop_unreferenced, when a kept face references it (plain stores of 1).  Both flag arrays
// are scanned; counts go to the host.  emit: kept vertices and faces at their scanned
// positions, so both keep their original relative order; faces reindexed; index_map new ->
// old.
//
// Every grid is sized from an element count; every loop is over a host-given count or is
// the find chase above.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sdfr_common.h"
#include "sdfr_scan.h"

namespace sdfr {

namespace {

constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / 64;
constexpr int kCcSlot = 9;              // words of a wave's slot in the statistics kernels

#define CC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CC_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

inline uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }
inline uint32_t blocks_for(uint32_t n) { return (n + kCcThreads - 1) / kCcThreads; }

// the small region at the end of the workspace
struct CcMisc {
    uint32_t err;          // set to 1 by a kernel that met a bad index / component id
    uint32_t box[6];       // keys of the mesh's bounding box: min x y z, max x y z
    uint32_t pad;
    double unit;           // the area unit u
};

// workspace regions: Sv (V + 2) | block sums | Sf (F + 1) | block sums | CcMisc
struct CcWs {
    uint64_t bsv_off, sf_off, bsf_off, misc_off, bytes;
};

CcWs cc_ws(uint32_t V, uint32_t F) {
    CcWs w;
    w.bsv_off = up256(((uint64_t)V + 2) * sizeof(uint32_t));
    w.sf_off = w.bsv_off + up256((uint64_t)scan_block_sums(V) * sizeof(uint32_t) + 4);
    w.bsf_off = w.sf_off + up256(((uint64_t)F + 1) * sizeof(uint32_t));
    w.misc_off = w.bsf_off + up256((uint64_t)scan_block_sums(F) * sizeof(uint32_t) + 4);
    w.bytes = w.misc_off + up256(sizeof(CcMisc));
    return w;
}

bool sizes_ok(uint32_t V, uint32_t F) {
    return V != 0 && V < (1u << 31) && 3ull * F < (1ull << 31);
}

// ------------------------------------------------------------------------------ labelling
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t x) {
    int32_t curr = CC_LOAD(parent + x);
    if (curr != x) {
        int32_t prev = x, next;
        while (curr > (next = CC_LOAD(parent + curr))) {
            CC_STORE(parent + prev, next);         // path halving
            prev = curr;
            curr = next;
        }
    }
    return curr;
}

__device__ __forceinline__ void cc_union(int32_t *parent, int32_t a, int32_t b) {
    int32_t ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        const bool a_hi = ra > rb;
        const int32_t hi = a_hi ? ra : rb, lo = a_hi ? rb : ra;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        // another thread lowered hi (old < hi): go on from what it hooked hi under
        const int32_t r = cc_find(parent, old);
        if (a_hi) ra = r; else rb = r;
    }
}

__device__ __forceinline__ bool face_ok(const int32_t *faces, uint32_t f, uint32_t V, int32_t &a,
                                        int32_t &b, int32_t &c) {
    a = faces[3ull * f];
    b = faces[3ull * f + 1];
    c = faces[3ull * f + 2];
    return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;
}

__global__ void __launch_bounds__(kCcThreads) cc_init_kernel(int32_t *parent, uint32_t V) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v < V) parent[v] = (int32_t)v;
}

__global__ void __launch_bounds__(kCcThreads) cc_union_kernel(const int32_t *faces, uint32_t V,
                                                            uint32_t F, int32_t *parent,
                                                            uint32_t *err) {
    const uint32_t f = blockIdx.x * kCcThreads + threadIdx.x;
    if (f >= F) return;
    int32_t a, b, c;
    if (!face_ok(faces, f, V, a, b, c)) {
        CC_STORE(err, 1u);
        return;
    }
    cc_union(parent, a, b);
    cc_union(parent, b, c);
}

__global__ void __launch_bounds__(kCcThreads) cc_flatten_kernel(int32_t *label, uint32_t V) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v >= V) return;
    int32_t r = (int32_t)v, p;
    while ((p = CC_LOAD(label + r)) < r) r = p;
    CC_STORE(label + v, r);
}

__global__ void __launch_bounds__(kCcThreads) cc_root_flag_kernel(const int32_t *label, uint32_t V,
                                                                uint32_t *S) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v < V) S[v] = label[v] == (int32_t)v ? 1u : 0u;
}

__global__ void __launch_bounds__(kCcThreads) cc_rank_kernel(const int32_t *label, uint32_t V,
                                                           const uint32_t *S, int32_t *comp) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t r = (uint32_t)label[v];
    comp[v] = r < V ? (int32_t)S[r] : 0;          // (r < V by construction)
}

// ------------------------------------------------------------------------------ statistics
// order-preserving image of a float: a < b (as floats, -0 < +0) <=> key(a) < key(b)
__device__ __forceinline__ uint32_t f2key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// Whether the valid lanes of this wave (all 64 lanes are active here) hold one component id.
// first: the lowest valid lane; n: the number of valid lanes.
__device__ __forceinline__ bool wave_uniform(bool valid, uint32_t c, uint32_t &first,
                                             uint32_t &n, uint32_t &cref) {
    const uint64_t mask = __ballot(valid);
    n = (uint32_t)__popcll(mask);
    first = mask ? (uint32_t)__ffsll((long long)mask) - 1u : 0u;
    cref = (uint32_t)__shfl((int)c, (int)first);
    return __ballot(valid && c != cref) == 0;
}

__global__ void __launch_bounds__(kCcThreads) cc_stats_init_kernel(uint32_t C, uint32_t *n_vertices,
                                                                 uint32_t *n_faces, uint32_t *box,
                                                                 uint64_t *area_q, CcMisc *misc) {
    const uint32_t c = blockIdx.x * kCcThreads + threadIdx.x;
    if (c < C) {
        n_vertices[c] = 0;
        n_faces[c] = 0;
        area_q[c] = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            box[6ull * c + q] = 0xffffffffu;
            box[6ull * c + 3 + q] = 0u;
        }
    }
    if (c == 0) {
        misc->err = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            misc->box[q] = 0xffffffffu;
            misc->box[3 + q] = 0u;
        }
        misc->unit = 1.0;
    }
}

// The waves of this block that hold anything agree on one component id (slot q of sh:
// [0] the wave's id, [1] its number of valid lanes, [2] whether it is uniform).  n: the
// block's number of valid threads.
__device__ __forceinline__ bool block_uniform(const uint32_t (*sh)[kCcSlot], uint32_t &n,
                                              uint32_t &cref) {
    bool uni = true;
    n = 0;
    cref = 0;
#pragma unroll
    for (int q = 0; q < kCcWaves; ++q) {
        if (sh[q][1] == 0) continue;
        if (n == 0) cref = sh[q][0];
        uni = uni && sh[q][2] != 0 && sh[q][0] == cref;
        n += sh[q][1];
    }
    return uni;
}

// one thread per vertex: count and component box.  One atomic per statistic per block when
// the block holds one component, per wave when the wave does, else per lane.
__global__ void __launch_bounds__(kCcThreads) cc_stats_vertex_kernel(
    const float *verts, const int32_t *comp, uint32_t V, uint32_t C, uint32_t *n_vertices,
    uint32_t *box, CcMisc *misc) {
    __shared__ uint32_t sh[kCcWaves][kCcSlot];
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    bool valid = v < V;
    uint32_t c = 0, k[3] = {0, 0, 0};
    if (valid) {
        c = (uint32_t)comp[v];
        if (c >= C) {
            CC_STORE(&misc->err, 1u);
            valid = false;
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) k[q] = f2key(verts[3ull * v + q]);
        }
    }
    uint32_t first, n, cref;
    const bool uni = wave_uniform(valid, c, first, n, cref);
    uint32_t lo[3], hi[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        lo[q] = wave_min(valid ? k[q] : 0xffffffffu);
        hi[q] = wave_max(valid ? k[q] : 0u);
    }
    if (lane == 0) {
        sh[w][0] = cref;
        sh[w][1] = n;
        sh[w][2] = uni ? 1u : 0u;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            sh[w][3 + q] = lo[q];
            sh[w][6 + q] = hi[q];
        }
    }
    __syncthreads();
    uint32_t bn, bc;
    if (block_uniform(sh, bn, bc)) {                 // (block-uniform branch)
        if (threadIdx.x != 0 || bn == 0) return;
        atomicAdd(&n_vertices[bc], bn);
#pragma unroll
        for (int q = 0; q < 3; ++q) {                // (a wave without valid lanes: identities)
            uint32_t l = sh[0][3 + q], h = sh[0][6 + q];
#pragma unroll
            for (int r = 1; r < kCcWaves; ++r) {
                l = min(l, sh[r][3 + q]);
                h = max(h, sh[r][6 + q]);
            }
            atomicMin(&box[6ull * bc + q], l);
            atomicMax(&box[6ull * bc + 3 + q], h);
        }
    } else if (uni) {                                // (wave-uniform branch)
        if (n == 0 || lane != first) return;
        atomicAdd(&n_vertices[cref], n);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            atomicMin(&box[6ull * cref + q], lo[q]);
            atomicMax(&box[6ull * cref + 3 + q], hi[q]);
        }
    } else if (valid) {
        atomicAdd(&n_vertices[c], 1u);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            atomicMin(&box[6ull * c + q], k[q]);
            atomicMax(&box[6ull * c + 3 + q], k[q]);
        }
    }
}

// one thread per component: the mesh's box from the components' boxes (keys), one atomic
// per extreme per wave
__global__ void __launch_bounds__(kCcThreads) cc_stats_meshbox_kernel(const uint32_t *box,
                                                                    uint32_t C, CcMisc *misc) {
    const uint32_t c = blockIdx.x * kCcThreads + threadIdx.x;
    const bool valid = c < C;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const uint32_t l = wave_min(valid ? box[6ull * c + q] : 0xffffffffu);
        const uint32_t h = wave_max(valid ? box[6ull * c + 3 + q] : 0u);
        if ((threadIdx.x & 63u) == 0) {
            atomicMin(&misc->box[q], l);
            atomicMax(&misc->box[3 + q], h);
        }
    }
}

// one thread: the area unit from the mesh's box and F (the rule of the header comment)
__global__ void cc_stats_unit_kernel(uint32_t F, CcMisc *misc) {
    double d = 0.0;
    for (int q = 0; q < 3; ++q) {
        const double e = (double)key2f(misc->box[3 + q]) - (double)key2f(misc->box[q]);
        d = e > d ? e : d;                           // (a NaN edge is skipped)
    }
    const double x = 2.0 * d * d * (double)(F ? F : 1u);
    double u = 1.0;
    if (x > 0.0 && x <= 1.7e308) {
        int k;
        frexp(x, &k);
        u = ldexp(1.0, k - 61);
    }
    misc->unit = u;
}

// one thread per face: count and area, reduced like the vertex kernel's statistics
__global__ void __launch_bounds__(kCcThreads) cc_stats_face_kernel(
    const float *verts, const int32_t *faces, const int32_t *comp, uint32_t V, uint32_t F,
    uint32_t C, uint32_t *n_faces, uint64_t *area_q, CcMisc *misc) {
    __shared__ uint32_t sh[kCcWaves][kCcSlot];
    const uint32_t f = blockIdx.x * kCcThreads + threadIdx.x;
    bool valid = f < F;
    uint32_t c = 0;
    uint64_t q = 0;
    if (valid) {
        int32_t a, b, cc;
        if (!face_ok(faces, f, V, a, b, cc) || (c = (uint32_t)comp[a]) >= C) {
            CC_STORE(&misc->err, 1u);
            valid = false;
        } else {
            double p[3][3];
            const int32_t id[3] = {a, b, cc};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) p[r][s] = (double)verts[3ull * (uint32_t)id[r] + s];
            const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double nx = e1[1] * e2[2] - e1[2] * e2[1];
            const double ny = e1[2] * e2[0] - e1[0] * e2[2];
            const double nz = e1[0] * e2[1] - e1[1] * e2[0];
            const double area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
            const double s = area / misc->unit;
            // (NaN compares false: 0)
            q = s >= 2305843009213693952.0 ? (1ull << 61) : s > 0.0 ? (uint64_t)llrint(s) : 0ull;
        }
    }
    uint32_t first, n, cref;
    const bool uni = wave_uniform(valid, c, first, n, cref);
    const uint64_t sum = wave_sum64(valid ? q : 0ull);
    if ((threadIdx.x & 63u) == 0) {
        uint32_t *slot = sh[threadIdx.x >> 6];
        slot[0] = cref;
        slot[1] = n;
        slot[2] = uni ? 1u : 0u;
        slot[3] = (uint32_t)sum;
        slot[4] = (uint32_t)(sum >> 32);
    }
    __syncthreads();
    uint32_t bn, bc;
    if (block_uniform(sh, bn, bc)) {                 // (block-uniform branch)
        if (threadIdx.x != 0 || bn == 0) return;
        uint64_t total = 0;
#pragma unroll
        for (int r = 0; r < kCcWaves; ++r) total += ((uint64_t)sh[r][4] << 32) | sh[r][3];
        atomicAdd(&n_faces[bc], bn);
        atomicAdd((unsigned long long *)&area_q[bc], (unsigned long long)total);
    } else if (uni) {                                // (wave-uniform branch)
        if (n == 0 || (threadIdx.x & 63u) != first) return;
        atomicAdd(&n_faces[cref], n);
        atomicAdd((unsigned long long *)&area_q[cref], (unsigned long long)sum);
    } else if (valid) {
        atomicAdd(&n_faces[c], 1u);
        atomicAdd((unsigned long long *)&area_q[c], (unsigned long long)q);
    }
}

__global__ void __launch_bounds__(kCcThreads) cc_stats_decode_kernel(uint32_t n, uint32_t *box) {
    const uint32_t i = blockIdx.x * kCcThreads + threadIdx.x;
    if (i < n) box[i] = __float_as_uint(key2f(box[i]));
}

// ------------------------------------------------------------------------------- selection
__global__ void __launch_bounds__(kCcThreads) cc_select_vertex_kernel(const int32_t *comp,
                                                                    const uint8_t *keep, uint32_t V,
                                                                    uint32_t C, uint32_t *Sv,
                                                                    uint32_t *err) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t c = (uint32_t)comp[v];
    if (c >= C) {
        CC_STORE(err, 1u);
        Sv[v] = 0;
        return;
    }
    Sv[v] = keep[c] ? 1u : 0u;
}

// Sv is zero before this kernel when drop is set, and holds the vertex flags otherwise
__global__ void __launch_bounds__(kCcThreads) cc_select_face_kernel(
    const int32_t *faces, const int32_t *comp, const uint8_t *keep, uint32_t V, uint32_t F,
    uint32_t C, int drop, uint32_t *Sv, uint32_t *Sf, uint32_t *err) {
    const uint32_t f = blockIdx.x * kCcThreads + threadIdx.x;
    if (f >= F) return;
    int32_t a, b, c;
    uint32_t k = 0;
    if (!face_ok(faces, f, V, a, b, c)) {
        CC_STORE(err, 1u);
    } else {
        const uint32_t id = (uint32_t)comp[a];
        if (id >= C) {
            CC_STORE(err, 1u);
        } else if (keep[id]) {
            k = 1;
            if (drop) Sv[a] = Sv[b] = Sv[c] = 1u;
        }
    }
    Sf[f] = k;
}

__global__ void __launch_bounds__(kCcThreads) cc_emit_vertex_kernel(const float *verts, uint32_t V,
                                                                  const uint32_t *Sv, uint32_t Vout,
                                                                  float *verts_out,
                                                                  int32_t *index_map) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t o = Sv[v];
    if (Sv[v + 1u] == o || o >= Vout) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) verts_out[3ull * o + q] = verts[3ull * v + q];
    index_map[o] = (int32_t)v;
}

__global__ void __launch_bounds__(kCcThreads) cc_emit_face_kernel(const int32_t *faces, uint32_t V,
                                                                uint32_t F, const uint32_t *Sv,
                                                                const uint32_t *Sf, uint32_t Fout,
                                                                int32_t *faces_out) {
    const uint32_t f = blockIdx.x * kCcThreads + threadIdx.x;
    if (f >= F) return;
    const uint32_t o = Sf[f];
    if (Sf[f + 1u] == o || o >= Fout) return;
    int32_t a, b, c;
    const bool ok = face_ok(faces, f, V, a, b, c);   // (a kept face was valid at the count)
    faces_out[3ull * o] = ok ? (int32_t)Sv[a] : 0;
    faces_out[3ull * o + 1] = ok ? (int32_t)Sv[b] : 0;
    faces_out[3ull * o + 2] = ok ? (int32_t)Sv[c] : 0;
}

int cc_setup(const char *what, uint32_t V, uint32_t F, const void *ws, size_t ws_bytes, CcWs &w) {
    if (!sizes_ok(V, F))
        return fail(SDFR_EINVAL, std::string(what) + ": V must be in [1, 2^31) and 3 F below 2^31");
    if (!ws) return fail(SDFR_EINVAL, std::string(what) + ": null workspace");
    w = cc_ws(V, F);
    if (ws_bytes < w.bytes) return fail(SDFR_EINVAL, std::string(what) + ": workspace too small");
    return SDFR_OK;
}

}  // namespace

}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_mesh_cc_workspace_bytes(uint32_t V, uint32_t F) {
    if (!sizes_ok(V, F)) return 0;
    return (size_t)cc_ws(V, F).bytes;
}

extern "C" int sdfr_mesh_cc_label(const int32_t *faces, uint32_t V, uint32_t F, int32_t *label,
                                  int32_t *comp, void *ws, size_t ws_bytes,
                                  uint32_t *n_components, void *stream) {
    if ((!faces && F) || !label || !comp || !n_components)
        return fail(SDFR_EINVAL, "mesh_cc_label: null faces / label / comp / n_components");
    CcWs w;
    int rc = cc_setup("mesh_cc_label", V, F, ws, ws_bytes, w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *S = (uint32_t *)ws;                    // [V + 2]: S[V] the total, S[V + 1] the error
    uint32_t *bsum = (uint32_t *)((char *)ws + w.bsv_off);
    if (hipMemsetAsync(S + V + 1, 0, sizeof(uint32_t), st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_cc_label: clearing the error word");
    cc_init_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(label, V);
    if (F) cc_union_kernel<<<blocks_for(F), kCcThreads, 0, st>>>(faces, V, F, label, S + V + 1);
    cc_flatten_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(label, V);
    cc_root_flag_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(label, V, S);
    exclusive_scan_u32(S, V, bsum, st);
    cc_rank_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(label, V, S, comp);
    rc = check_launch("mesh_cc_label");
    if (rc) return rc;
    uint32_t tail[2];
    if (hipMemcpyAsync(tail, S + V, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_cc_label: reading the count");
    if (tail[1]) return fail(SDFR_EINVAL, "mesh_cc_label: a face index is outside [0, V)");
    *n_components = tail[0];
    return SDFR_OK;
}

extern "C" int sdfr_mesh_cc_stats(const float *verts, const int32_t *faces, const int32_t *comp,
                                  uint32_t V, uint32_t F, uint32_t C, uint32_t *n_vertices,
                                  uint32_t *n_faces, float *bbox, uint64_t *area_q,
                                  double *area_unit, void *ws, size_t ws_bytes, void *stream) {
    if (!verts || (!faces && F) || !comp || !n_vertices || !n_faces || !bbox || !area_q ||
        !area_unit)
        return fail(SDFR_EINVAL, "mesh_cc_stats: null verts / faces / comp / output");
    CcWs w;
    int rc = cc_setup("mesh_cc_stats", V, F, ws, ws_bytes, w);
    if (rc) return rc;
    if (C == 0 || C > V) return fail(SDFR_EINVAL, "mesh_cc_stats: C must be in [1, V]");
    hipStream_t st = (hipStream_t)stream;
    CcMisc *misc = (CcMisc *)((char *)ws + w.misc_off);
    uint32_t *box = (uint32_t *)bbox;
    cc_stats_init_kernel<<<blocks_for(C), kCcThreads, 0, st>>>(C, n_vertices, n_faces, box, area_q,
                                                              misc);
    cc_stats_vertex_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(verts, comp, V, C, n_vertices,
                                                                box, misc);
    cc_stats_meshbox_kernel<<<blocks_for(C), kCcThreads, 0, st>>>(box, C, misc);
    cc_stats_unit_kernel<<<1, 1, 0, st>>>(F, misc);
    if (F)
        cc_stats_face_kernel<<<blocks_for(F), kCcThreads, 0, st>>>(verts, faces, comp, V, F, C,
                                                                  n_faces, area_q, misc);
    cc_stats_decode_kernel<<<blocks_for(6u * C), kCcThreads, 0, st>>>(6u * C, box);
    rc = check_launch("mesh_cc_stats");
    if (rc) return rc;
    CcMisc h;
    if (hipMemcpyAsync(&h, misc, sizeof(CcMisc), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_cc_stats: reading the unit");
    if (h.err)
        return fail(SDFR_EINVAL, "mesh_cc_stats: a face index is outside [0, V) or a component "
                                 "id outside [0, C)");
    *area_unit = h.unit;
    return SDFR_OK;
}

extern "C" int sdfr_mesh_cc_select_count(const int32_t *faces, const int32_t *comp,
                                         const uint8_t *keep, uint32_t V, uint32_t F, uint32_t C,
                                         int drop_unreferenced, void *ws, size_t ws_bytes,
                                         uint32_t *counts, void *stream) {
    if ((!faces && F) || !comp || !keep || !counts)
        return fail(SDFR_EINVAL, "mesh_cc_select: null faces / comp / keep / counts");
    CcWs w;
    int rc = cc_setup("mesh_cc_select", V, F, ws, ws_bytes, w);
    if (rc) return rc;
    if (C == 0 || C > V) return fail(SDFR_EINVAL, "mesh_cc_select: C must be in [1, V]");
    hipStream_t st = (hipStream_t)stream;
    uint32_t *Sv = (uint32_t *)ws, *Sf = (uint32_t *)((char *)ws + w.sf_off);
    uint32_t *bsv = (uint32_t *)((char *)ws + w.bsv_off);
    uint32_t *bsf = (uint32_t *)((char *)ws + w.bsf_off);
    uint32_t *err = &((CcMisc *)((char *)ws + w.misc_off))->err;
    const bool drop = drop_unreferenced != 0;
    if (hipMemsetAsync(err, 0, sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(Sf, 0, ((size_t)F + 1) * sizeof(uint32_t), st) != hipSuccess ||
        (drop && hipMemsetAsync(Sv, 0, ((size_t)V + 1) * sizeof(uint32_t), st) != hipSuccess))
        return fail(SDFR_ELAUNCH, "mesh_cc_select: clearing the flags");
    if (!drop)
        cc_select_vertex_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(comp, keep, V, C, Sv, err);
    if (F)
        cc_select_face_kernel<<<blocks_for(F), kCcThreads, 0, st>>>(faces, comp, keep, V, F, C,
                                                                   drop ? 1 : 0, Sv, Sf, err);
    exclusive_scan_u32(Sv, V, bsv, st);
    if (F) exclusive_scan_u32(Sf, F, bsf, st);
    rc = check_launch("mesh_cc_select: count");
    if (rc) return rc;
    uint32_t tail[3];
    if (hipMemcpyAsync(tail, Sv + V, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(tail + 1, Sf + F, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(tail + 2, err, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_cc_select: reading the counts");
    if (tail[2])
        return fail(SDFR_EINVAL, "mesh_cc_select: a face index is outside [0, V) or a component "
                                 "id outside [0, C)");
    counts[0] = tail[0];
    counts[1] = tail[1];
    return SDFR_OK;
}

extern "C" int sdfr_mesh_cc_select_emit(const float *verts, const int32_t *faces, uint32_t V,
                                        uint32_t F, uint32_t V_out, uint32_t F_out, const void *ws,
                                        size_t ws_bytes, float *verts_out, int32_t *faces_out,
                                        int32_t *index_map, void *stream) {
    if (!verts || (!faces && F) || !verts_out || (!faces_out && F_out) || !index_map)
        return fail(SDFR_EINVAL, "mesh_cc_select: null verts / faces / output");
    CcWs w;
    int rc = cc_setup("mesh_cc_select", V, F, ws, ws_bytes, w);
    if (rc) return rc;
    if (V_out == 0 || V_out > V || F_out > F)
        return fail(SDFR_EINVAL, "mesh_cc_select: V_out must be in [1, V] and F_out in [0, F]");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t *Sv = (const uint32_t *)ws;
    const uint32_t *Sf = (const uint32_t *)((const char *)ws + w.sf_off);
    cc_emit_vertex_kernel<<<blocks_for(V), kCcThreads, 0, st>>>(verts, V, Sv, V_out, verts_out,
                                                               index_map);
    if (F && F_out)
        cc_emit_face_kernel<<<blocks_for(F), kCcThreads, 0, st>>>(faces, V, F, Sv, Sf, F_out,
                                                                 faces_out);
    return check_launch("mesh_cc_select: emit");
}

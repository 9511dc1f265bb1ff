// mesh_simplify.hip -- vertex-clustering simplification of an indexed triangle mesh on the
// device (include/sdfr.h, "Mesh simplification"; DESIGN.md "Mesh simplification"): cell of
// every vertex, clusters, cluster positions, face deduplication, compaction.
//
// Every output is a pure function of the mesh and the grid: the only order-dependent
// operations are integer atomics whose results do not depend on the order (CAS claims of a
// slot whose class never changes afterwards, atomicMin, atomicAdd on integers).
//
// Cell table.  Open addressing with linear probing, capacity the power of two >= 2 V (load
// <= 1/2).  A slot is a 64-bit key (all ones = empty; a key fits 63 bits) and a 32-bit
// value (all ones at the start).  A vertex probes from the hash of its key: atomicCAS(key
// slot, empty, key) returns empty (claimed) or the occupant's key; on its own key it stops
// and lowers the value with atomicMin(value, v), otherwise it probes on.  A claimed slot
// keeps its key for good, so all vertices of a cell end in one slot, and the slot's value
// ends as the smallest of their indices, whatever the schedule: rep.
//
// Numbering.  is_rep[v] = (rep[v] == v), the exclusive scan of sdfr_scan.h, cluster id =
// rank[rep[v]]: ids 0..C-1 in increasing order of rep.
//
// Sums.  S_x, S_y, S_z (the quantised offsets q inside the cell, 20 fractional bits) and the
// member count m by 64-bit integer atomicAdd on four consecutive words per cluster.  When
// the valid lanes of a wave hold one cluster the wave reduces with shuffles and one lane
// issues the four atomics (20 000 vertices in one cell are then 313 atomics per word, not
// 20 000); otherwise every lane issues its own.  Both add the same integers.
//
// Face table.  Capacity the power of two >= 2 F, slots hold a face index (all ones =
// empty).  A face whose corners map to three distinct clusters probes from the hash of its
// sorted cluster triple: atomicCAS(slot, empty, f) claims; on an occupant it reads the
// occupant's triple (faces and cluster ids are read-only here) -- the same triple:
// atomicMin(slot, f) and stop, another: probe on.  The class of a slot never changes once
// claimed, so a class lives in exactly one slot, which ends holding the smallest face index
// of the class.  A face is kept when that slot holds its own index.
//
// Finish.  Cluster flags (all C, or with drop_unreferenced those a kept face references) and
// face flags are scanned; emit writes kept clusters and faces at their scanned positions, so
// both keep their relative order.
//
// Validation.  A face index outside [0, V) or a non-finite coordinate is never used to
// address memory: the element is skipped and a bit of the device error word is set, which
// the count call reads back with its counts.
//
// Every grid is sized from an element count; every probe loop is bounded by the table's
// capacity (which it cannot reach: the tables are at most half full).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sdfr_common.h"
#include "sdfr_scan.h"

namespace sdfr {

namespace {

constexpr int kSimpThreads = 256;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint32_t kMaxDim = 1u << 21;
constexpr uint32_t kErrFace = 1u, kErrFinite = 2u, kErrTable = 4u;

inline uint64_t sp_up256(uint64_t v) { return (v + 255) & ~255ull; }
inline uint32_t sp_blocks(uint32_t n) { return (n + kSimpThreads - 1) / kSimpThreads; }
inline uint64_t pow2_ceil(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the small region at the end of the workspace: the error word and the grid, which emit
// reads back (its call does not repeat the grid)
struct SpMisc {
    uint32_t err;
    uint32_t n[3];
    float o[3];
    float cell;
};

// Workspace regions.  Set to all ones: vkeys (Cv u64) | vvals (Cv u32) | ftab (Cf u32).
// Set to zero: sums (4 u64 per vertex) | Su (V + 1) | misc.  Written before read: A (V) |
// Sv (V + 1) | fslot (F) | Sf (F + 1) | the scans' block sums.
struct SpWs {
    uint64_t cv, cf;
    uint64_t vvals_off, ftab_off, ones_end, sums_off, su_off, misc_off, zero_end, a_off, sv_off,
        fslot_off, sf_off, bsv_off, bsu_off, bsf_off, bytes;
};

SpWs sp_ws(uint32_t V, uint32_t F) {
    SpWs w;
    w.cv = pow2_ceil(2ull * V);
    w.cf = pow2_ceil(F ? 2ull * F : 1ull);
    w.vvals_off = w.cv * sizeof(uint64_t);
    w.ftab_off = w.vvals_off + sp_up256(w.cv * sizeof(uint32_t));
    w.ones_end = w.ftab_off + sp_up256(w.cf * sizeof(uint32_t));
    w.sums_off = w.ones_end;
    w.su_off = w.sums_off + sp_up256(4ull * V * sizeof(uint64_t));
    w.misc_off = w.su_off + sp_up256(((uint64_t)V + 1) * sizeof(uint32_t));
    w.zero_end = w.misc_off + sp_up256(sizeof(SpMisc));
    w.a_off = w.zero_end;
    w.sv_off = w.a_off + sp_up256((uint64_t)V * sizeof(uint32_t));
    w.fslot_off = w.sv_off + sp_up256(((uint64_t)V + 1) * sizeof(uint32_t));
    w.sf_off = w.fslot_off + sp_up256((uint64_t)F * sizeof(uint32_t));
    w.bsv_off = w.sf_off + sp_up256(((uint64_t)F + 1) * sizeof(uint32_t));
    w.bsu_off = w.bsv_off + sp_up256((uint64_t)scan_block_sums(V) * sizeof(uint32_t) + 4);
    w.bsf_off = w.bsu_off + sp_up256((uint64_t)scan_block_sums(V) * sizeof(uint32_t) + 4);
    w.bytes = w.bsf_off + sp_up256((uint64_t)scan_block_sums(F) * sizeof(uint32_t) + 4);
    return w;
}

bool sp_sizes_ok(uint32_t V, uint32_t F) {
    return V != 0 && V < (1u << 31) && 3ull * F < (1ull << 31);
}

// ------------------------------------------------------------------------ the definition
__device__ __forceinline__ bool finite3(const float (&p)[3]) {
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// per axis: t = (v - o) / cell, c = clamp(floor(t), 0, n - 1) (as float), q = rint(clamp(t -
// c, 0, 1) 2^20); one rounded fp32 operation each
__device__ __forceinline__ void cell_of(float v, float o, float cell, uint32_t n, uint32_t &c,
                                        uint32_t &q) {
    const float t = __fdiv_rn(__fsub_rn(v, o), cell);
    const float cf = fminf(fmaxf(floorf(t), 0.0f), (float)(n - 1u));
    const float r = fminf(fmaxf(__fsub_rn(t, cf), 0.0f), 1.0f);
    c = (uint32_t)cf;
    q = (uint32_t)rintf(__fmul_rn(r, 1048576.0f));
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ void load3(const float *verts, uint32_t v, float (&p)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = verts[3ull * v + k];
}

__device__ __forceinline__ bool sp_face_ok(const int32_t *faces, uint32_t f, uint32_t V,
                                           uint32_t &a, uint32_t &b, uint32_t &c) {
    a = (uint32_t)faces[3ull * f];
    b = (uint32_t)faces[3ull * f + 1];
    c = (uint32_t)faces[3ull * f + 2];
    return a < V && b < V && c < V;
}

__device__ __forceinline__ void sort3(uint32_t &a, uint32_t &b, uint32_t &c) {
    uint32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

// ------------------------------------------------------------------------------ clusters
__global__ void sp_params_kernel(SpMisc *misc, float ox, float oy, float oz, float cell,
                                 uint32_t nx, uint32_t ny, uint32_t nz) {
    misc->o[0] = ox;
    misc->o[1] = oy;
    misc->o[2] = oz;
    misc->cell = cell;
    misc->n[0] = nx;
    misc->n[1] = ny;
    misc->n[2] = nz;
}

// one thread per vertex: claim or find the slot of its cell, lower the slot's value to v.
// A[v] = the slot.
__global__ void __launch_bounds__(kSimpThreads) sp_insert_kernel(
    const float *verts, uint32_t V, const SpMisc *misc, unsigned long long *vkeys,
    uint32_t *vvals, uint64_t cv, uint32_t *A, uint32_t *err) {
    const uint32_t v = blockIdx.x * kSimpThreads + threadIdx.x;
    if (v >= V) return;
    float p[3];
    load3(verts, v, p);
    if (!finite3(p)) {
        atomicOr(err, kErrFinite);
        A[v] = 0;                                    // (any slot: its value is range-checked)
        return;
    }
    uint32_t c[3], q;
#pragma unroll
    for (int k = 0; k < 3; ++k) cell_of(p[k], misc->o[k], misc->cell, misc->n[k], c[k], q);
    const uint64_t key = ((uint64_t)c[0] * misc->n[1] + c[1]) * misc->n[2] + c[2];
    const uint64_t mask = cv - 1;
    uint64_t i = mix64(key) & mask;
    for (uint64_t step = 0; step < cv; ++step, i = (i + 1) & mask) {
        const uint64_t old = atomicCAS(vkeys + i, (unsigned long long)kEmptyKey,
                                       (unsigned long long)key);
        if (old == kEmptyKey || old == key) {
            atomicMin(vvals + i, v);
            A[v] = (uint32_t)i;
            return;
        }
    }
    atomicOr(err, kErrTable);                        // (unreachable: the table is half empty)
    A[v] = 0;
}

// A[v]: slot -> rep; Sv[v] = is_rep
__global__ void __launch_bounds__(kSimpThreads) sp_rep_kernel(const uint32_t *vvals, uint32_t V,
                                                             uint32_t *A, uint32_t *Sv) {
    const uint32_t v = blockIdx.x * kSimpThreads + threadIdx.x;
    if (v >= V) return;
    uint32_t r = vvals[A[v]];
    if (r >= V) r = v;                               // (a skipped vertex: its own cluster)
    A[v] = r;
    Sv[v] = r == v ? 1u : 0u;
}

__device__ __forceinline__ uint64_t sp_wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// A[v]: rep -> cluster id (Sv scanned); the cluster's sums
__global__ void __launch_bounds__(kSimpThreads) sp_sums_kernel(const float *verts, uint32_t V,
                                                              const SpMisc *misc,
                                                              const uint32_t *Sv, uint32_t *A,
                                                              unsigned long long *sums) {
    const uint32_t v = blockIdx.x * kSimpThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool valid = v < V;
    uint32_t g = 0;
    uint64_t q[4] = {0, 0, 0, 1};
    if (valid) {
        g = Sv[A[v]];                                // (A[v] < V by construction)
        A[v] = g;
        float p[3];
        load3(verts, v, p);
        if (finite3(p)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint32_t c, qq;
                cell_of(p[k], misc->o[k], misc->cell, misc->n[k], c, qq);
                q[k] = qq;
            }
        } else {
            valid = false;
        }
    }
    // (all 64 lanes are active here)
    const uint64_t vmask = __ballot(valid);
    if (vmask == 0) return;
    const uint32_t first = (uint32_t)__ffsll((long long)vmask) - 1u;
    const uint32_t gref = (uint32_t)__shfl((int)g, (int)first);
    if (__ballot(valid && g != gref) == 0) {         // (wave-uniform branch)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t s = sp_wave_sum64(valid ? q[k] : 0ull);
            if (lane == first) atomicAdd(sums + 4ull * gref + k, (unsigned long long)s);
        }
    } else if (valid) {
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(sums + 4ull * g + k, (unsigned long long)q[k]);
    }
}

// --------------------------------------------------------------------------------- faces
// cluster triple of face f, sorted; false for a bad index (when given, *bad is set) or two
// equal corners
__device__ __forceinline__ bool face_triple(const int32_t *faces, const uint32_t *A, uint32_t f,
                                            uint32_t V, uint32_t (&g)[3], bool *bad) {
    uint32_t a, b, c;
    if (!sp_face_ok(faces, f, V, a, b, c)) {
        if (bad) *bad = true;
        return false;
    }
    g[0] = A[a];
    g[1] = A[b];
    g[2] = A[c];
    if (g[0] == g[1] || g[1] == g[2] || g[0] == g[2]) return false;
    sort3(g[0], g[1], g[2]);
    return true;
}

// one thread per face: fslot[f] = the slot of its class, or none
__global__ void __launch_bounds__(kSimpThreads) sp_face_insert_kernel(
    const int32_t *faces, const uint32_t *A, uint32_t V, uint32_t F, uint32_t *ftab, uint64_t cf,
    uint32_t *fslot, uint32_t *err) {
    const uint32_t f = blockIdx.x * kSimpThreads + threadIdx.x;
    if (f >= F) return;
    uint32_t g[3];
    bool bad = false;
    if (!face_triple(faces, A, f, V, g, &bad)) {
        if (bad) atomicOr(err, kErrFace);
        fslot[f] = kNone;
        return;
    }
    const uint64_t mask = cf - 1;
    uint64_t i = mix64((((uint64_t)g[0] << 32) | g[1]) ^
                       mix64((uint64_t)g[2] + 0x9e3779b97f4a7c15ull)) & mask;
    for (uint64_t step = 0; step < cf; ++step, i = (i + 1) & mask) {
        const uint32_t occ = atomicCAS(ftab + i, kNone, f);
        if (occ == kNone) {
            fslot[f] = (uint32_t)i;
            return;
        }
        uint32_t h[3];
        // (an occupant is a face that passed face_triple; occ < F guards the read anyway)
        if (occ < F && face_triple(faces, A, occ, V, h, nullptr) && h[0] == g[0] &&
            h[1] == g[1] && h[2] == g[2]) {
            atomicMin(ftab + i, f);
            fslot[f] = (uint32_t)i;
            return;
        }
    }
    atomicOr(err, kErrTable);                        // (unreachable: the table is half empty)
    fslot[f] = kNone;
}

// Sf[f] = kept; with drop, the clusters of a kept face are flagged (Su is zero before)
__global__ void __launch_bounds__(kSimpThreads) sp_face_keep_kernel(
    const int32_t *faces, const uint32_t *A, uint32_t V, uint32_t F, const uint32_t *ftab,
    const uint32_t *fslot, int drop, uint32_t *Su, uint32_t *Sf) {
    const uint32_t f = blockIdx.x * kSimpThreads + threadIdx.x;
    if (f >= F) return;
    const uint32_t s = fslot[f];
    const bool kept = s != kNone && ftab[s] == f;
    Sf[f] = kept ? 1u : 0u;
    if (kept && drop) {
        uint32_t a, b, c;
        if (sp_face_ok(faces, f, V, a, b, c)) Su[A[a]] = Su[A[b]] = Su[A[c]] = 1u;
    }
}

// without drop: every cluster is kept
__global__ void __launch_bounds__(kSimpThreads) sp_keep_all_kernel(const uint32_t *Sv, uint32_t V,
                                                                  uint32_t *Su) {
    const uint32_t v = blockIdx.x * kSimpThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t g = Sv[v];
    if (Sv[v + 1u] != g) Su[g] = 1u;
}

// ---------------------------------------------------------------------------------- emit
__global__ void __launch_bounds__(kSimpThreads) sp_emit_vertex_kernel(
    const float *verts, uint32_t V, const SpMisc *misc, const uint32_t *A, const uint32_t *Sv,
    const uint32_t *Su, const unsigned long long *sums, uint32_t Vout, float *verts_out,
    int32_t *index_map, int32_t *cluster, uint32_t *members) {
    const uint32_t v = blockIdx.x * kSimpThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t g = A[v];
    if (g >= V) return;                              // (a workspace the count did not fill)
    const uint32_t o = Su[g];
    const bool kept = Su[g + 1u] != o && o < Vout;
    if (cluster) cluster[v] = kept ? (int32_t)o : -1;
    if (!kept || Sv[v + 1u] == Sv[v]) return;        // only the rep writes the cluster
    float p[3];
    load3(verts, v, p);
    const uint64_t m = sums[4ull * g + 3];
    const double den = __dmul_rn((double)m, 1048576.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t c, q;
        cell_of(p[k], misc->o[k], misc->cell, misc->n[k], c, q);
        const double mean = __ddiv_rn((double)(int64_t)sums[4ull * g + k], den);
        const double x = __dadd_rn((double)misc->o[k],
                                   __dmul_rn(__dadd_rn((double)c, mean), (double)misc->cell));
        verts_out[3ull * o + k] = (float)x;
    }
    index_map[o] = (int32_t)v;
    if (members) members[o] = (uint32_t)m;
}

__global__ void __launch_bounds__(kSimpThreads) sp_emit_face_kernel(
    const int32_t *faces, const uint32_t *A, uint32_t V, uint32_t F, const uint32_t *Su,
    const uint32_t *Sf, uint32_t Fout, int32_t *faces_out) {
    const uint32_t f = blockIdx.x * kSimpThreads + threadIdx.x;
    if (f >= F) return;
    const uint32_t o = Sf[f];
    if (Sf[f + 1u] == o || o >= Fout) return;
    uint32_t a, b, c;
    const bool ok = sp_face_ok(faces, f, V, a, b, c);  // (a kept face was valid at the count)
    const uint32_t ga = ok ? A[a] : 0u, gb = ok ? A[b] : 0u, gc = ok ? A[c] : 0u;
    faces_out[3ull * o] = ga < V ? (int32_t)Su[ga] : 0;
    faces_out[3ull * o + 1] = gb < V ? (int32_t)Su[gb] : 0;
    faces_out[3ull * o + 2] = gc < V ? (int32_t)Su[gc] : 0;
}

int sp_setup(uint32_t V, uint32_t F, const void *ws, size_t ws_bytes, SpWs &w) {
    if (!sp_sizes_ok(V, F))
        return fail(SDFR_EINVAL, "mesh_simplify: V must be in [1, 2^31) and 3 F below 2^31");
    if (!ws) return fail(SDFR_EINVAL, "mesh_simplify: null workspace");
    w = sp_ws(V, F);
    if (ws_bytes < w.bytes) return fail(SDFR_EINVAL, "mesh_simplify: workspace too small");
    return SDFR_OK;
}

}  // namespace

}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_mesh_simplify_workspace_bytes(uint32_t V, uint32_t F) {
    if (!sp_sizes_ok(V, F)) return 0;
    return (size_t)sp_ws(V, F).bytes;
}

extern "C" int sdfr_mesh_simplify_count(const float *verts, const int32_t *faces, uint32_t V,
                                        uint32_t F, float ox, float oy, float oz, float cell,
                                        uint32_t nx, uint32_t ny, uint32_t nz,
                                        int drop_unreferenced, void *ws, size_t ws_bytes,
                                        uint32_t *counts, void *stream) {
    if (!verts || (!faces && F) || !counts)
        return fail(SDFR_EINVAL, "mesh_simplify: null verts / faces / counts");
    if (!std::isfinite(cell) || !(cell > 0.0f))
        return fail(SDFR_EINVAL, "mesh_simplify: cell must be finite and > 0");
    if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz))
        return fail(SDFR_EINVAL, "mesh_simplify: the origin must be finite");
    if (nx == 0 || ny == 0 || nz == 0 || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim)
        return fail(SDFR_EINVAL, "mesh_simplify: nx, ny, nz must be in [1, 2^21]");
    SpWs w;
    int rc = sp_setup(V, F, ws, ws_bytes, w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    unsigned long long *vkeys = (unsigned long long *)base;
    uint32_t *vvals = (uint32_t *)(base + w.vvals_off);
    uint32_t *ftab = (uint32_t *)(base + w.ftab_off);
    unsigned long long *sums = (unsigned long long *)(base + w.sums_off);
    uint32_t *Su = (uint32_t *)(base + w.su_off);
    SpMisc *misc = (SpMisc *)(base + w.misc_off);
    uint32_t *A = (uint32_t *)(base + w.a_off);
    uint32_t *Sv = (uint32_t *)(base + w.sv_off);
    uint32_t *fslot = (uint32_t *)(base + w.fslot_off);
    uint32_t *Sf = (uint32_t *)(base + w.sf_off);
    uint32_t *bsv = (uint32_t *)(base + w.bsv_off);
    uint32_t *bsu = (uint32_t *)(base + w.bsu_off);
    uint32_t *bsf = (uint32_t *)(base + w.bsf_off);
    const int drop = drop_unreferenced != 0 ? 1 : 0;
    if (hipMemsetAsync(base, 0xff, (size_t)w.ones_end, st) != hipSuccess ||
        hipMemsetAsync(base + w.ones_end, 0, (size_t)(w.zero_end - w.ones_end), st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_simplify: clearing the tables");
    sp_params_kernel<<<1, 1, 0, st>>>(misc, ox, oy, oz, cell, nx, ny, nz);
    sp_insert_kernel<<<sp_blocks(V), kSimpThreads, 0, st>>>(verts, V, misc, vkeys, vvals, w.cv, A,
                                                           &misc->err);
    sp_rep_kernel<<<sp_blocks(V), kSimpThreads, 0, st>>>(vvals, V, A, Sv);
    exclusive_scan_u32(Sv, V, bsv, st);
    sp_sums_kernel<<<sp_blocks(V), kSimpThreads, 0, st>>>(verts, V, misc, Sv, A, sums);
    if (F) {
        sp_face_insert_kernel<<<sp_blocks(F), kSimpThreads, 0, st>>>(faces, A, V, F, ftab, w.cf,
                                                                    fslot, &misc->err);
        sp_face_keep_kernel<<<sp_blocks(F), kSimpThreads, 0, st>>>(faces, A, V, F, ftab, fslot,
                                                                  drop, Su, Sf);
    }
    if (!drop) sp_keep_all_kernel<<<sp_blocks(V), kSimpThreads, 0, st>>>(Sv, V, Su);
    exclusive_scan_u32(Su, V, bsu, st);
    if (F) exclusive_scan_u32(Sf, F, bsf, st);
    rc = check_launch("mesh_simplify: count");
    if (rc) return rc;
    uint32_t tail[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(tail, Sv + V, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(tail + 1, Su + V, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        (F && hipMemcpyAsync(tail + 2, Sf + F, sizeof(uint32_t), hipMemcpyDeviceToHost, st) !=
                  hipSuccess) ||
        hipMemcpyAsync(tail + 3, &misc->err, sizeof(uint32_t), hipMemcpyDeviceToHost, st) !=
            hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_simplify: reading the counts");
    if (tail[3] & kErrFace) return fail(SDFR_EINVAL, "mesh_simplify: a face index is outside [0, V)");
    if (tail[3] & kErrFinite)
        return fail(SDFR_EINVAL, "mesh_simplify: a vertex coordinate is not finite");
    if (tail[3]) return fail(SDFR_ELAUNCH, "mesh_simplify: a table overflowed");
    counts[0] = tail[0];
    counts[1] = tail[1];
    counts[2] = tail[2];
    return SDFR_OK;
}

extern "C" int sdfr_mesh_simplify_emit(const float *verts, const int32_t *faces, uint32_t V,
                                       uint32_t F, uint32_t V_out, uint32_t F_out, const void *ws,
                                       size_t ws_bytes, float *verts_out, int32_t *faces_out,
                                       int32_t *index_map, int32_t *cluster, uint32_t *members,
                                       void *stream) {
    if (!verts || (!faces && F) || !verts_out || (!faces_out && F_out) || !index_map)
        return fail(SDFR_EINVAL, "mesh_simplify: null verts / faces / output");
    SpWs w;
    int rc = sp_setup(V, F, ws, ws_bytes, w);
    if (rc) return rc;
    if (V_out == 0 || V_out > V || F_out > F)
        return fail(SDFR_EINVAL, "mesh_simplify: V_out must be in [1, V] and F_out in [0, F]");
    hipStream_t st = (hipStream_t)stream;
    const char *base = (const char *)ws;
    const unsigned long long *sums = (const unsigned long long *)(base + w.sums_off);
    const uint32_t *Su = (const uint32_t *)(base + w.su_off);
    const SpMisc *misc = (const SpMisc *)(base + w.misc_off);
    const uint32_t *A = (const uint32_t *)(base + w.a_off);
    const uint32_t *Sv = (const uint32_t *)(base + w.sv_off);
    const uint32_t *Sf = (const uint32_t *)(base + w.sf_off);
    sp_emit_vertex_kernel<<<sp_blocks(V), kSimpThreads, 0, st>>>(
        verts, V, misc, A, Sv, Su, sums, V_out, verts_out, index_map, cluster, members);
    if (F && F_out)
        sp_emit_face_kernel<<<sp_blocks(F), kSimpThreads, 0, st>>>(faces, A, V, F, Su, Sf, F_out,
                                                                  faces_out);
    return check_launch("mesh_simplify: emit");
}

// mesh_smooth.hip -- Laplacian / Taubin smoothing of an indexed triangle mesh on the device
// (include/sdfr.h, "Mesh smoothing"; DESIGN.md "Mesh smoothing"): quantise the vertices to an
// integer lattice, build every vertex's row of neighbours once, run Jacobi passes on the
// integer state, de-quantise.
//
// Every output is a pure function of the mesh, the lattice and the weights: the state is
// int32, a pass sums in int64 (any order gives the same sum), and the only atomics are integer
// ones whose results do not depend on the order (valence counts, CAS claims of an edge slot
// whose key never changes afterwards, counts per slot).  The order of a row's entries does
// depend on the schedule, and nothing reads it: a row is only ever summed.
//
// Prepare.
//   quantise   one thread per vertex: q = rint(((double)v - (double)o) / u) per axis into
//              Q0[v] = (qx, qy, qz, 0), 16 bytes.
//   count      one thread per face: the valence of its three corners (atomicAdd), and its
//              edge slots into the edge table.  Edge table: open addressing, linear probing,
//              capacity the power of two >= 4 F (at most 3 F distinct pairs: never full), a
//              slot is a 64-bit key (min << 32 | max, never 0; 0 = empty) and a 32-bit count.
//              atomicCAS(key slot, empty, key) returns empty (claimed) or the occupant's key;
//              on its own key the slot's count goes up by one, otherwise it probes on.
//   boundary   one thread per table slot: a slot whose count is exactly 1 flags both ends.
//   scan       the valences (sdfr_scan.h) -> R[v], the first corner of vertex v's row.
//   fill       one thread per face: each corner takes the next free place of its vertex's row
//              (atomicAdd on a cursor) and writes the face's other two corners there, 8 bytes.
//   flags      one thread per vertex: Q0[v].w = movable; the valence and boundary outputs.
//
// Pass.  A gather: one thread per vertex reads Q[v], walks its row, reads Q[a] and Q[b] (16
// bytes each) and writes Q'[v]; no atomics, ping-pong between two buffers (the first pass
// reads Q0, which a run never writes, so every run starts from the prepared state).  A row of
// more than kLongRow corners is not walked by its own lane: after the short rows, the wave
// takes its long rows one at a time, all 64 lanes striding over the row's corners and
// reducing with shuffles -- the fan hub costs its wave valence / 64 steps, and no workgroup
// barrier waits on it (the kernel has none).
//
// Finish.  verts_out[v] = verts[v] for a vertex that was never movable (and for all of them
// after 0 passes), otherwise (float)((double)o + (double)q u).
//
// Validation.  A face index outside [0, V), a non-finite coordinate or a vertex outside the
// lattice is never used to address memory: the element is skipped (the same test in count
// and fill, so a row holds valid indices only) and a bit of the device error word is set,
// which prepare reads back.
//
// Every grid is sized from an element count; the probe loop is bounded by the table's
// capacity; a row's extent comes from the scanned valences, which the same faces filled.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sdfr_common.h"
#include "sdfr_scan.h"

namespace sdfr {

namespace {

constexpr int kSmThreads = 256;
constexpr uint32_t kLongRow = 32;                    // corners; longer rows: the whole wave
constexpr uint32_t kMaxPasses = 1024;
constexpr int kUnitLog2Min = -126, kUnitLog2Max = 96;  // u a normal fp32, 2^31 u finite
constexpr unsigned long long kSmEmptyKey = 0ull;     // (a key's low word, the larger index, is >= 1)
constexpr uint32_t kSmErrFace = 1u, kSmErrFinite = 2u, kSmErrLattice = 4u, kSmErrTable = 8u;
constexpr int64_t kQMax = 1ll << 30;                 // inputs lie in [0, kQMax]
constexpr int64_t kClampLo = -(1ll << 30), kClampHi = (1ll << 31) - 1;

inline uint64_t sm_up256(uint64_t v) { return (v + 255) & ~255ull; }
inline uint32_t sm_blocks(uint64_t n) { return (uint32_t)((n + kSmThreads - 1) / kSmThreads); }
inline uint64_t sm_pow2_ceil(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the small region of the workspace that run reads back on the device: the lattice
struct SmMisc {
    uint32_t err;
    int unit_log2;
    float o[3];
};

// Workspace regions.  First what depends on V alone, so that run finds it without F.  Set to
// zero: R (V + 1 u32) | cursor (V u32) | bflag (V bytes) | misc.  Written before read: Q0,
// QA, QB (V int4 each) | the scan's block sums | rows (3 F uint2).  Set to zero: ecnt (Ce
// u32) | ekeys (Ce u64).
struct SmWs {
    uint64_t ce;
    uint64_t r_off, cur_off, bflag_off, misc_off, zero_end, q0_off, qa_off, qb_off, bs_off,
        rows_off, ecnt_off, ekeys_off, bytes;
};

SmWs sm_ws(uint32_t V, uint32_t F) {
    SmWs w;
    w.ce = sm_pow2_ceil(F ? 4ull * F : 1ull);
    w.r_off = 0;
    w.cur_off = w.r_off + sm_up256(((uint64_t)V + 1) * sizeof(uint32_t));
    w.bflag_off = w.cur_off + sm_up256((uint64_t)V * sizeof(uint32_t));
    w.misc_off = w.bflag_off + sm_up256((uint64_t)V);
    w.zero_end = w.misc_off + sm_up256(sizeof(SmMisc));
    w.q0_off = w.zero_end;
    w.qa_off = w.q0_off + sm_up256(16ull * V);
    w.qb_off = w.qa_off + sm_up256(16ull * V);
    w.bs_off = w.qb_off + sm_up256(16ull * V);
    w.rows_off = w.bs_off + sm_up256((uint64_t)scan_block_sums(V) * sizeof(uint32_t) + 4);
    w.ecnt_off = w.rows_off + sm_up256(24ull * F);
    w.ekeys_off = w.ecnt_off + sm_up256(w.ce * sizeof(uint32_t));
    w.bytes = w.ekeys_off + sm_up256(w.ce * sizeof(uint64_t));
    return w;
}

bool sm_sizes_ok(uint32_t V, uint32_t F) {
    return V != 0 && V < (1u << 31) && 3ull * F < (1ull << 31);
}

// ------------------------------------------------------------------------ the definition
__device__ __forceinline__ uint64_t sm_mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ bool sm_face_ok(const int32_t *faces, uint32_t f, uint32_t V,
                                           uint32_t (&c)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (uint32_t)faces[3ull * f + k];
    return c[0] < V && c[1] < V && c[2] < V;
}

// q' = clamp(q + rint((w D) / (2 d)), ...): one conversion, one product, one quotient, rint
// (|S| <= 2 d (2^31 - 1) fits int64 for every d < 2^31; D = S - 2 d q for d <= 2^30, the
// definition's limit)
__device__ __forceinline__ int32_t sm_step(int32_t q, int64_t S, uint32_t d, double w) {
    const int64_t D = S - 2ll * (int64_t)d * (int64_t)q;
    const double t = __ddiv_rn(__dmul_rn(w, (double)D), (double)(2ull * d));
    int64_t n = (int64_t)q + (int64_t)rint(t);
    n = n < kClampLo ? kClampLo : (n > kClampHi ? kClampHi : n);
    return (int32_t)n;
}

__device__ __forceinline__ int64_t sm_wave_sum64(int64_t x) {
    uint64_t v = (uint64_t)x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        v += ((uint64_t)hi << 32) | lo;
    }
    return (int64_t)v;
}

// ------------------------------------------------------------------------------- prepare
__global__ void sm_params_kernel(SmMisc *misc, float ox, float oy, float oz, int unit_log2) {
    misc->o[0] = ox;
    misc->o[1] = oy;
    misc->o[2] = oz;
    misc->unit_log2 = unit_log2;
}

__global__ void __launch_bounds__(kSmThreads) sm_quantise_kernel(const float *verts, uint32_t V,
                                                                 float ox, float oy, float oz,
                                                                 int unit_log2, int4 *Q0,
                                                                 uint32_t *err) {
    const uint32_t v = blockIdx.x * kSmThreads + threadIdx.x;
    if (v >= V) return;
    const float o[3] = {ox, oy, oz};
    int q[3] = {0, 0, 0};
    uint32_t e = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = verts[3ull * v + k];
        if (!isfinite(p)) {
            e |= kSmErrFinite;
            continue;
        }
        // (the scaling by a power of two is exact: |v - o| < 2^129, 2^-96 <= 1 / u <= 2^126)
        const double t = rint(ldexp(__dsub_rn((double)p, (double)o[k]), -unit_log2));
        if (t >= 0.0 && t <= (double)kQMax)
            q[k] = (int)t;
        else
            e |= kSmErrLattice;
    }
    if (e) atomicOr(err, e);
    Q0[v] = make_int4(q[0], q[1], q[2], 0);
}

// one thread per face: valences into R, edge slots into the table
__global__ void __launch_bounds__(kSmThreads) sm_count_kernel(const int32_t *faces, uint32_t V,
                                                              uint32_t F, uint32_t *R,
                                                              unsigned long long *ekeys,
                                                              uint32_t *ecnt, uint64_t ce,
                                                              uint32_t *err) {
    const uint32_t f = blockIdx.x * kSmThreads + threadIdx.x;
    if (f >= F) return;
    uint32_t c[3];
    if (!sm_face_ok(faces, f, V, c)) {
        atomicOr(err, kSmErrFace);
        return;
    }
    const uint64_t mask = ce - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicAdd(R + c[k], 1u);
        const uint32_t a = c[k], b = c[k == 2 ? 0 : k + 1];
        if (a == b) continue;
        const unsigned long long key =
            ((unsigned long long)(a < b ? a : b) << 32) | (unsigned long long)(a < b ? b : a);
        uint64_t i = sm_mix64(key) & mask;
        bool placed = false;
        for (uint64_t step = 0; step < ce; ++step, i = (i + 1) & mask) {
            const unsigned long long old = atomicCAS(ekeys + i, kSmEmptyKey, key);
            if (old == kSmEmptyKey || old == key) {
                atomicAdd(ecnt + i, 1u);
                placed = true;
                break;
            }
        }
        if (!placed) atomicOr(err, kSmErrTable);     // (unreachable: 3 F pairs, >= 4 F slots)
    }
}

// one thread per table slot: a pair of multiplicity exactly 1 flags both its ends
__global__ void __launch_bounds__(kSmThreads) sm_boundary_kernel(const unsigned long long *ekeys,
                                                                 const uint32_t *ecnt, uint64_t ce,
                                                                 uint32_t V, uint8_t *bflag) {
    const uint64_t i = (uint64_t)blockIdx.x * kSmThreads + threadIdx.x;
    if (i >= ce) return;
    const unsigned long long key = ekeys[i];
    if (key == kSmEmptyKey || ecnt[i] != 1u) return;
    const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
    if (a < V && b < V) bflag[a] = bflag[b] = 1;     // (a key holds two valid indices)
}

__global__ void __launch_bounds__(kSmThreads) sm_copy_valence_kernel(const uint32_t *R, uint32_t V,
                                                                     int32_t *valence) {
    const uint32_t v = blockIdx.x * kSmThreads + threadIdx.x;
    if (v < V) valence[v] = (int32_t)R[v];
}

// one thread per face (R scanned): each corner's entry (the other two, as written)
__global__ void __launch_bounds__(kSmThreads) sm_fill_kernel(const int32_t *faces, uint32_t V,
                                                             uint32_t F, const uint32_t *R,
                                                             uint32_t *cursor, uint2 *rows) {
    const uint32_t f = blockIdx.x * kSmThreads + threadIdx.x;
    if (f >= F) return;
    uint32_t c[3];
    if (!sm_face_ok(faces, f, V, c)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t at = R[c[k]] + atomicAdd(cursor + c[k], 1u);
        if (at < R[c[k] + 1u] && at < 3ull * F)      // (always: the count saw the same faces)
            rows[at] = make_uint2(c[(k + 1) % 3], c[(k + 2) % 3]);
    }
}

__global__ void __launch_bounds__(kSmThreads) sm_flags_kernel(const uint32_t *R,
                                                              const uint8_t *bflag, uint32_t V,
                                                              int pin, int4 *Q0,
                                                              uint8_t *boundary) {
    const uint32_t v = blockIdx.x * kSmThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t d = R[v + 1u] - R[v];
    const uint8_t b = bflag[v];
    Q0[v].w = (d > 0 && !(pin && b)) ? 1 : 0;
    if (boundary) boundary[v] = b;
}

// ---------------------------------------------------------------------------------- pass
__global__ void __launch_bounds__(kSmThreads) sm_pass_kernel(const int4 *__restrict__ src,
                                                             int4 *__restrict__ dst,
                                                             const uint32_t *__restrict__ R,
                                                             const uint2 *__restrict__ rows,
                                                             uint32_t V, uint64_t n_rows,
                                                             double w) {
    const uint32_t v = blockIdx.x * kSmThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = v < V;                        // (no early return: the wave works together)
    int4 q = make_int4(0, 0, 0, 0);
    uint32_t r0 = 0, d = 0;
    if (valid) {
        q = src[v];
        r0 = R[v];
        const uint32_t r1 = R[v + 1u];
        // (a workspace that prepare did not fill: no row leaves the rows region)
        d = (r1 >= r0 && r1 <= n_rows) ? r1 - r0 : 0u;
    }
    const bool movable = valid && q.w != 0 && d > 0;
    const bool is_long = movable && d > kLongRow;
    int64_t S[3] = {0, 0, 0};
    if (movable && !is_long) {
        for (uint32_t k = 0; k < d; ++k) {
            const uint2 e = rows[(uint64_t)r0 + k];
            if (e.x >= V || e.y >= V) continue;      // (never: rows hold valid indices)
            const int4 a = src[e.x], b = src[e.y];
            S[0] += (int64_t)a.x + (int64_t)b.x;
            S[1] += (int64_t)a.y + (int64_t)b.y;
            S[2] += (int64_t)a.z + (int64_t)b.z;
        }
    }
    // the wave's long rows, one at a time, 64 corners per step (all 64 lanes are active here)
    uint64_t todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t lr0 = (uint32_t)__shfl((int)r0, owner);
        const uint32_t ld = (uint32_t)__shfl((int)d, owner);
        int64_t P[3] = {0, 0, 0};
        for (uint32_t k = lane; k < ld; k += 64u) {
            const uint2 e = rows[(uint64_t)lr0 + k];
            if (e.x >= V || e.y >= V) continue;
            const int4 a = src[e.x], b = src[e.y];
            P[0] += (int64_t)a.x + (int64_t)b.x;
            P[1] += (int64_t)a.y + (int64_t)b.y;
            P[2] += (int64_t)a.z + (int64_t)b.z;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t s = sm_wave_sum64(P[k]);
            if ((int)lane == owner) S[k] = s;
        }
    }
    if (!valid) return;
    if (movable) {
        q.x = sm_step(q.x, S[0], d, w);
        q.y = sm_step(q.y, S[1], d, w);
        q.z = sm_step(q.z, S[2], d, w);
    }
    dst[v] = q;
}

// -------------------------------------------------------------------------------- finish
__global__ void __launch_bounds__(kSmThreads) sm_finish_kernel(const float *verts,
                                                               const int4 *Q, uint32_t V,
                                                               const SmMisc *misc, int moved,
                                                               float *verts_out) {
    const uint32_t v = blockIdx.x * kSmThreads + threadIdx.x;
    if (v >= V) return;
    const int4 q = Q[v];
    if (!moved || q.w == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) verts_out[3ull * v + k] = verts[3ull * v + k];
        return;
    }
    int ul = misc->unit_log2;
    ul = ul < kUnitLog2Min ? kUnitLog2Min : (ul > kUnitLog2Max ? kUnitLog2Max : ul);
    const int qq[3] = {q.x, q.y, q.z};
#pragma unroll
    for (int k = 0; k < 3; ++k)                      // (q u is exact in fp64)
        verts_out[3ull * v + k] =
            (float)__dadd_rn((double)misc->o[k], ldexp((double)qq[k], ul));
}

int sm_setup(uint32_t V, uint32_t F, const void *ws, size_t ws_bytes, SmWs &w) {
    if (!sm_sizes_ok(V, F))
        return fail(SDFR_EINVAL, "mesh_smooth: V must be in [1, 2^31) and 3 F below 2^31");
    if (!ws) return fail(SDFR_EINVAL, "mesh_smooth: null workspace");
    w = sm_ws(V, F);
    if (ws_bytes < w.bytes) return fail(SDFR_EINVAL, "mesh_smooth: workspace too small");
    return SDFR_OK;
}

}  // namespace

}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_mesh_smooth_workspace_bytes(uint32_t V, uint32_t F) {
    if (!sm_sizes_ok(V, F)) return 0;
    return (size_t)sm_ws(V, F).bytes;
}

extern "C" int sdfr_mesh_smooth_prepare(const float *verts, const int32_t *faces, uint32_t V,
                                        uint32_t F, float ox, float oy, float oz, int unit_log2,
                                        int pin_boundary, void *ws, size_t ws_bytes,
                                        int32_t *valence, uint8_t *boundary, void *stream) {
    if (!verts || (!faces && F)) return fail(SDFR_EINVAL, "mesh_smooth: null verts / faces");
    if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz))
        return fail(SDFR_EINVAL, "mesh_smooth: the origin must be finite");
    if (unit_log2 < kUnitLog2Min || unit_log2 > kUnitLog2Max)
        return fail(SDFR_EINVAL, "mesh_smooth: unit_log2 must be in [-126, 96]");
    SmWs w;
    int rc = sm_setup(V, F, ws, ws_bytes, w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    unsigned long long *ekeys = (unsigned long long *)(base + w.ekeys_off);
    uint32_t *ecnt = (uint32_t *)(base + w.ecnt_off);
    uint32_t *R = (uint32_t *)(base + w.r_off);
    uint32_t *cursor = (uint32_t *)(base + w.cur_off);
    uint8_t *bflag = (uint8_t *)(base + w.bflag_off);
    SmMisc *misc = (SmMisc *)(base + w.misc_off);
    int4 *Q0 = (int4 *)(base + w.q0_off);
    uint2 *rows = (uint2 *)(base + w.rows_off);
    uint32_t *bs = (uint32_t *)(base + w.bs_off);
    if (hipMemsetAsync(base, 0, (size_t)w.zero_end, st) != hipSuccess ||
        hipMemsetAsync(base + w.ecnt_off, 0, (size_t)(w.bytes - w.ecnt_off), st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_smooth: clearing the tables");
    sm_params_kernel<<<1, 1, 0, st>>>(misc, ox, oy, oz, unit_log2);
    sm_quantise_kernel<<<sm_blocks(V), kSmThreads, 0, st>>>(verts, V, ox, oy, oz, unit_log2, Q0,
                                                           &misc->err);
    if (F) {
        sm_count_kernel<<<sm_blocks(F), kSmThreads, 0, st>>>(faces, V, F, R, ekeys, ecnt, w.ce,
                                                            &misc->err);
        sm_boundary_kernel<<<sm_blocks(w.ce), kSmThreads, 0, st>>>(ekeys, ecnt, w.ce, V, bflag);
    }
    if (valence) sm_copy_valence_kernel<<<sm_blocks(V), kSmThreads, 0, st>>>(R, V, valence);
    exclusive_scan_u32(R, V, bs, st);
    if (F) sm_fill_kernel<<<sm_blocks(F), kSmThreads, 0, st>>>(faces, V, F, R, cursor, rows);
    sm_flags_kernel<<<sm_blocks(V), kSmThreads, 0, st>>>(R, bflag, V, pin_boundary != 0 ? 1 : 0,
                                                        Q0, boundary);
    rc = check_launch("mesh_smooth: prepare");
    if (rc) return rc;
    uint32_t err = 0;
    if (hipMemcpyAsync(&err, &misc->err, sizeof(uint32_t), hipMemcpyDeviceToHost, st) !=
            hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_smooth: reading the error word");
    if (err & kSmErrFace) return fail(SDFR_EINVAL, "mesh_smooth: a face index is outside [0, V)");
    if (err & kSmErrFinite)
        return fail(SDFR_EINVAL, "mesh_smooth: a vertex coordinate is not finite");
    if (err & kSmErrLattice)
        return fail(SDFR_EINVAL, "mesh_smooth: a vertex is outside the lattice");
    if (err) return fail(SDFR_ELAUNCH, "mesh_smooth: the edge table overflowed");
    return SDFR_OK;
}

extern "C" int sdfr_mesh_smooth_run(const float *verts, uint32_t V, const float *weights,
                                    uint32_t n_passes, const void *ws, size_t ws_bytes,
                                    float *verts_out, void *stream) {
    if (!verts || !verts_out || (!weights && n_passes))
        return fail(SDFR_EINVAL, "mesh_smooth: null verts / weights / verts_out");
    if (n_passes > kMaxPasses) return fail(SDFR_EINVAL, "mesh_smooth: n_passes must be <= 1024");
    for (uint32_t p = 0; p < n_passes; ++p)
        if (!std::isfinite(weights[p]) || std::fabs(weights[p]) > 1.0f)
            return fail(SDFR_EINVAL, "mesh_smooth: a weight must be finite with |w| <= 1");
    SmWs w;
    int rc = sm_setup(V, 0, ws, ws_bytes, w);        // (what run reads starts at offsets of V)
    if (rc) return rc;
    const uint64_t max_rows = (ws_bytes - w.rows_off) / sizeof(uint2);
    const char *vb = (const char *)verts, *ob = (const char *)verts_out;
    if (vb < ob + 12ull * V && ob < vb + 12ull * V)
        return fail(SDFR_EINVAL, "mesh_smooth: verts_out must not alias verts");
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;                         // (run writes the ping-pong buffers only)
    const SmMisc *misc = (const SmMisc *)(base + w.misc_off);
    const uint32_t *R = (const uint32_t *)(base + w.r_off);
    const uint2 *rows = (const uint2 *)(base + w.rows_off);
    const int4 *Q0 = (const int4 *)(base + w.q0_off);
    int4 *pp[2] = {(int4 *)(base + w.qa_off), (int4 *)(base + w.qb_off)};
    const int4 *cur = Q0;
    for (uint32_t p = 0; p < n_passes; ++p) {
        int4 *next = pp[p & 1u];
        sm_pass_kernel<<<sm_blocks(V), kSmThreads, 0, st>>>(cur, next, R, rows, V, max_rows,
                                                           (double)weights[p]);
        cur = next;
    }
    sm_finish_kernel<<<sm_blocks(V), kSmThreads, 0, st>>>(verts, cur, V, misc,
                                                         n_passes != 0 ? 1 : 0, verts_out);
    return check_launch("mesh_smooth: run");
}

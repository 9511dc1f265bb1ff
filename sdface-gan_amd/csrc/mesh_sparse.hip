// mesh_sparse.hip -- marching cubes over narrow-band brick storage (include/sdfr.h,
// "Sparse marching cubes"; DESIGN.md "Narrow-band bricks").
//
// The grid of res^3 points is cut into 8^3-point bricks; only the bricks the surface can
// pass through are stored, values [n, 8, 8, 8] fp32 behind a slot table slots [nb^3].
// Cells belong to the brick of their low corner, and only the cells of `surface` bricks
// are triangulated; their corners reach into the bricks K + {0,1}^3, which the layout
// call stores as well.
//
//   sdfr_brick_layout     dilate surface -> needed, give the needed bricks without a slot
//                         the slots n_prev, n_prev + 1, ... in ascending brick index (one
//                         flag pass, the scan of sdfr_scan.h, one assign pass)
//   sdfr_brick_points     copy the axis tables' entries into the points of slots
//                         [slot0, slot1): no coordinate is computed here
//   sdfr_mc_sparse_count  one thread per stored point, lz fastest: the three edge flags
//                         (crossed, and an edge of a surface brick's cell), the cell's
//                         triangle count, and the leak flags; then the scan.  Per brick
//                         S = [flag_0 | flag_1 | flag_2] (1536), then one triangle count
//                         per point behind all bricks' flags (3 P + 512 slot + l), so ids
//                         run slot-major, then as in mesh.hip within a brick
//   sdfr_mc_sparse_emit   vertices by put_vertex (mc_vertex.h, shared with mesh.hip) in
//                         global index coordinates, triangles with the shared per-edge ids
//
// Neighbours across a brick face go through the slot table.  A brick's 9^3 corner block
// is NOT staged in LDS: each lane's corner loads along lz coalesce within the brick's 2 KB.
// Measured (profiles/sparse_mesh_kernels.txt): 30.6 M stored points of a 1024^3 sphere
// classify in 0.51 ms and emit in 0.53 ms, 60 G points/s against the dense kernel's 113;
// closing that gap would save 0.5 ms of a 17.5 ms call, so the simpler form stays.
//
// Every table lookup is bounds-checked: a slot outside [0, n_bricks) reads as NaN (never
// inside), a slot without a brick emits nothing -- inconsistent tables give a wrong mesh,
// not a wild access.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "mc_table.h"
#include "mc_vertex.h"
#include "sdfr_common.h"
#include "sdfr_scan.h"

namespace sdfr {

namespace {

constexpr int kSpThreads = 256;
constexpr uint32_t kBrick = 512;          // 8^3 points
constexpr uint32_t kNoBrick = 0xffffffffu;

struct SpVol {
    const float *values;       // [n_bricks, 8, 8, 8]
    const int32_t *slots;      // [nb^3]
    const uint8_t *surface;    // [nb^3]
    const uint32_t *brick_of;  // [n_bricks]: brick index of a slot, or kNoBrick
    uint32_t nb, res, n_bricks;
    uint32_t P;                // 512 n_bricks
    float level;
};

__device__ __forceinline__ uint32_t brick_index(const SpVol &m, uint32_t i, uint32_t j,
                                                uint32_t k) {
    return ((i >> 3) * m.nb + (j >> 3)) * m.nb + (k >> 3);
}

__device__ __forceinline__ uint32_t local_index(uint32_t i, uint32_t j, uint32_t k) {
    return ((i & 7u) << 6) | ((j & 7u) << 3) | (k & 7u);
}

// slot of the brick that holds point (i, j, k) (each < res), or >= n_bricks
__device__ __forceinline__ uint32_t slot_of(const SpVol &m, uint32_t i, uint32_t j, uint32_t k) {
    return (uint32_t)m.slots[brick_index(m, i, j, k)];
}

__device__ __forceinline__ float at(const SpVol &m, uint32_t i, uint32_t j, uint32_t k) {
    const uint32_t s = slot_of(m, i, j, k);
    if (s >= m.n_bricks) return NAN;
    return m.values[(size_t)s * kBrick + local_index(i, j, k)];
}

// the cell with low corner (i, j, k) exists (unsigned: i - 1 of i = 0 fails here) and its
// brick is triangulated
__device__ __forceinline__ bool cell_surface(const SpVol &m, uint32_t i, uint32_t j, uint32_t k) {
    const uint32_t hi = m.res - 2u;
    if (i > hi || j > hi || k > hi) return false;
    return m.surface[brick_index(m, i, j, k)] != 0;
}

// corner c = x + 2y + 4z of the cell with low corner (i, j, k)
__device__ __forceinline__ uint32_t cell_case(const SpVol &m, uint32_t i, uint32_t j, uint32_t k) {
    uint32_t cs = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        cs |= (at(m, i + (q & 1), j + ((q >> 1) & 1), k + (q >> 2)) < m.level ? 1u : 0u) << q;
    return cs;
}

struct SpPoint {
    uint32_t s, l, q;      // slot, local index, brick index
    uint32_t i, j, k;      // global point index
};

__device__ __forceinline__ bool decode(const SpVol &m, SpPoint &p) {
    const uint32_t t = blockIdx.x * kSpThreads + threadIdx.x;
    p.s = t >> 9;
    p.l = t & 511u;
    if (p.s >= m.n_bricks) return false;
    p.q = m.brick_of[p.s];
    if (p.q == kNoBrick) return true;
    const uint32_t bz = p.q % m.nb, r = p.q / m.nb;
    p.i = (r / m.nb) * 8u + (p.l >> 6);
    p.j = (r % m.nb) * 8u + ((p.l >> 3) & 7u);
    p.k = bz * 8u + (p.l & 7u);
    return true;
}

__global__ void __launch_bounds__(kSpThreads) sp_brick_of(const int32_t *slots, uint32_t nq,
                                                          uint32_t n_bricks, uint32_t *brick_of) {
    const uint32_t q = blockIdx.x * kSpThreads + threadIdx.x;
    if (q >= nq) return;
    const uint32_t s = (uint32_t)slots[q];
    if (s < n_bricks) brick_of[s] = q;
}

// the four corners of a cell's face (axis d, low or high side) are not all on one side
__device__ __forceinline__ bool face_mixed(uint32_t cs, int d, bool high) {
    const uint32_t mask = d == 0 ? 0x55u : d == 1 ? 0x33u : 0x0fu;
    const uint32_t f = (high ? cs >> (1u << d) : cs) & mask;
    return f != 0 && f != mask;
}

__global__ void __launch_bounds__(kSpThreads) sp_classify(const SpVol m, uint32_t *S,
                                                          uint8_t *grow) {
    SpPoint p;
    if (!decode(m, p)) return;
    const uint32_t e = p.s * 3u * kBrick + p.l, c = 3u * m.P + p.s * kBrick + p.l;
    uint32_t f0 = 0, f1 = 0, f2 = 0, nt = 0;
    if (p.q != kNoBrick) {
        const uint32_t i = p.i, j = p.j, k = p.k;
        // the cells around this point's three edges: low corner (i - a, j - b, k - c)
        const bool c000 = cell_surface(m, i, j, k);
        const bool c010 = cell_surface(m, i, j - 1, k), c001 = cell_surface(m, i, j, k - 1);
        const bool c100 = cell_surface(m, i - 1, j, k), c011 = cell_surface(m, i, j - 1, k - 1);
        const bool c101 = cell_surface(m, i - 1, j, k - 1), c110 = cell_surface(m, i - 1, j - 1, k);
        const bool in = m.values[(size_t)p.s * kBrick + p.l] < m.level;
        // an edge of a triangulated cell has both ends in stored bricks and lies in the grid
        if (c000 || c010 || c001 || c011) f0 = in != (at(m, i + 1, j, k) < m.level);
        if (c000 || c100 || c001 || c101) f1 = in != (at(m, i, j + 1, k) < m.level);
        if (c000 || c100 || c010 || c110) f2 = in != (at(m, i, j, k + 1) < m.level);
        if (c000) {
            const uint32_t cs = cell_case(m, i, j, k);
            nt = kMcNTri[cs];
            if (grow) {
                const uint32_t x[3] = {i, j, k};
#pragma unroll
                for (int d = 0; d < 3; ++d) {
#pragma unroll
                    for (int high = 0; high < 2; ++high) {
                        // the cell across: another brick only from a border point
                        if ((x[d] & 7u) != (high ? 7u : 0u)) continue;
                        uint32_t y[3] = {i, j, k};
                        y[d] = high ? x[d] + 1u : x[d] - 1u;
                        if (y[d] > m.res - 2u) continue;
                        const uint32_t qn = brick_index(m, y[0], y[1], y[2]);
                        if (!m.surface[qn] && face_mixed(cs, d, high)) grow[qn] = 1;
                    }
                }
            }
        }
    }
    S[e] = f0;
    S[e + kBrick] = f1;
    S[e + 2u * kBrick] = f2;
    S[c] = nt;
}

// S scanned: an element's flag / count is the difference to its successor (S[4 P] = total)
__global__ void __launch_bounds__(kSpThreads) sp_emit(const SpVol m, const uint32_t *S,
                                                      float *verts, int32_t *faces) {
    SpPoint p;
    if (!decode(m, p) || p.q == kNoBrick) return;
    const uint32_t i = p.i, j = p.j, k = p.k;
    const uint32_t e = p.s * 3u * kBrick + p.l, c = 3u * m.P + p.s * kBrick + p.l;
    const float v = m.values[(size_t)p.s * kBrick + p.l];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const uint32_t id = S[e + d * kBrick];
        if (S[e + d * kBrick + 1u] == id) continue;
        const float w = at(m, i + (d == 0), j + (d == 1), k + (d == 2));
        put_vertex(verts, id, i, j, k, d, v, w, m.level);
    }
    const uint32_t t0 = S[c] - S[3u * m.P], nt = S[c + 1u] - S[c];
    if (nt == 0) return;
    const uint32_t cs = cell_case(m, i, j, k);
    for (uint32_t t = 0; t < nt; ++t) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ed = kMcTri[cs][3 * t + r];
            const int d = ed >> 2, lo = ed & 1, hi = (ed >> 1) & 1;
            // offsets of the edge's low end: axis 0 edges (y, z), axis 1 (x, z), axis 2 (x, y)
            const uint32_t qi = i + (d == 0 ? 0u : (uint32_t)lo);
            const uint32_t qj = j + (d == 0 ? (uint32_t)lo : d == 1 ? 0u : (uint32_t)hi);
            const uint32_t qk = k + (d == 2 ? 0u : (uint32_t)hi);
            const uint32_t s = slot_of(m, qi, qj, qk);
            int32_t id = 0;
            if (s < m.n_bricks) id = (int32_t)S[s * 3u * kBrick + (uint32_t)d * kBrick + local_index(qi, qj, qk)];
            faces[3ull * (t0 + t) + r] = id;
        }
    }
}

// ---- layout ----
__global__ void __launch_bounds__(kSpThreads) sp_layout_flag(const uint8_t *surface,
                                                             const int32_t *slots, uint32_t nb,
                                                             uint32_t nq, uint32_t *S) {
    const uint32_t q = blockIdx.x * kSpThreads + threadIdx.x;
    if (q >= nq) return;
    const uint32_t bz = q % nb, r = q / nb, by = r % nb, bx = r / nb;
    bool needed = false;
#pragma unroll
    for (uint32_t o = 0; o < 8; ++o) {
        const uint32_t a = o & 1u, b = (o >> 1) & 1u, c = o >> 2;
        if (bx >= a && by >= b && bz >= c)
            needed = needed || surface[((bx - a) * nb + (by - b)) * nb + (bz - c)] != 0;
    }
    S[q] = (needed && slots[q] < 0) ? 1u : 0u;
}

__global__ void __launch_bounds__(kSpThreads) sp_layout_assign(int32_t *slots, uint32_t nq,
                                                               const uint32_t *S, uint32_t n_prev) {
    const uint32_t q = blockIdx.x * kSpThreads + threadIdx.x;
    if (q >= nq) return;
    if (S[q + 1u] != S[q]) slots[q] = (int32_t)(n_prev + S[q]);
}

// one wave per brick index; a brick with a slot in [slot0, slot1) writes its 512 points
__global__ void __launch_bounds__(kSpThreads) sp_brick_points(const int32_t *slots, uint32_t nb,
                                                              uint32_t nq, uint32_t slot0,
                                                              uint32_t slot1, const float *ax,
                                                              const float *ay, const float *az,
                                                              float *points) {
    const uint32_t q = blockIdx.x * (kSpThreads / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const uint32_t s = (uint32_t)slots[q];
    if (s < slot0 || s >= slot1) return;
    const uint32_t bz = q % nb, r = q / nb, by = r % nb, bx = r / nb;
    float *out = points + (size_t)(s - slot0) * kBrick * 3u;
    for (uint32_t l = threadIdx.x & 63u; l < kBrick; l += 64u) {
        out[3u * l + 0] = ax[bx * 8u + (l >> 6)];
        out[3u * l + 1] = ay[by * 8u + ((l >> 3) & 7u)];
        out[3u * l + 2] = az[bz * 8u + (l & 7u)];
    }
}

inline uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }

int grid_check(const char *what, uint32_t nb) {
    if (nb == 0 || nb > 256)
        return fail(SDFR_EINVAL, std::string(what) + ": nb must be in [1, 256]");
    return SDFR_OK;
}

// workspace regions of the sparse marching cubes: S (4 P + 1) | block sums | brick_of
struct SpWs {
    uint64_t M, bsum_off, brick_off, bytes;
};

SpWs sp_ws(uint32_t n_bricks) {
    SpWs w;
    w.M = 4ull * kBrick * n_bricks;
    w.bsum_off = up256((w.M + 1) * sizeof(uint32_t));
    w.brick_off = w.bsum_off + up256((uint64_t)scan_block_sums(w.M) * sizeof(uint32_t));
    w.bytes = w.brick_off + up256((uint64_t)n_bricks * sizeof(uint32_t));
    return w;
}

int sp_setup(const float *values, const int32_t *slots, const uint8_t *surface, uint32_t nb,
             uint32_t n_bricks, float level, const void *ws, size_t ws_bytes, SpVol &m, SpWs &w) {
    if (!values || !slots || !surface || !ws)
        return fail(SDFR_EINVAL, "mc_sparse: null values / slots / surface / workspace");
    int rc = grid_check("mc_sparse", nb);
    if (rc) return rc;
    if (n_bricks == 0) return fail(SDFR_EINVAL, "mc_sparse: no bricks");
    if (4ull * kBrick * n_bricks + 1 >= (1ull << 32))
        return fail(SDFR_EINVAL, "mc_sparse: too many bricks (4 * 512 n + 1 must fit 32 bits)");
    w = sp_ws(n_bricks);
    if (ws_bytes < w.bytes) return fail(SDFR_EINVAL, "mc_sparse: workspace too small");
    m = SpVol{values, slots, surface, (const uint32_t *)((const char *)ws + w.brick_off),
              nb, nb * 8u, n_bricks, kBrick * n_bricks, level};
    return SDFR_OK;
}

}  // namespace

}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_brick_layout_workspace_bytes(uint32_t nb) {
    if (nb == 0 || nb > 256) return 0;
    const uint64_t nq = (uint64_t)nb * nb * nb;
    return (size_t)(up256((nq + 1) * sizeof(uint32_t)) + scan_block_sums(nq) * sizeof(uint32_t));
}

extern "C" int sdfr_brick_layout(const uint8_t *surface, uint32_t nb, int32_t *slots,
                                 uint32_t n_prev, void *ws, size_t ws_bytes, uint32_t *n_total,
                                 void *stream) {
    if (!surface || !slots || !ws || !n_total)
        return fail(SDFR_EINVAL, "brick_layout: null surface / slots / workspace / n_total");
    int rc = grid_check("brick_layout", nb);
    if (rc) return rc;
    if (ws_bytes < sdfr_brick_layout_workspace_bytes(nb))
        return fail(SDFR_EINVAL, "brick_layout: workspace too small");
    const uint32_t nq = nb * nb * nb;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *S = (uint32_t *)ws;
    uint32_t *bsum = (uint32_t *)((char *)ws + up256(((uint64_t)nq + 1) * sizeof(uint32_t)));
    const uint32_t blocks = (nq + kSpThreads - 1) / kSpThreads;
    sp_layout_flag<<<blocks, kSpThreads, 0, st>>>(surface, slots, nb, nq, S);
    exclusive_scan_u32(S, nq, bsum, st);
    sp_layout_assign<<<blocks, kSpThreads, 0, st>>>(slots, nq, S, n_prev);
    rc = check_launch("brick_layout");
    if (rc) return rc;
    uint32_t added = 0;
    if (hipMemcpyAsync(&added, S + nq, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "brick_layout: reading the total");
    *n_total = n_prev + added;
    return SDFR_OK;
}

extern "C" int sdfr_brick_points(const int32_t *slots, uint32_t nb, uint32_t slot0, uint32_t slot1,
                                 const float *ax, const float *ay, const float *az, float *points,
                                 void *stream) {
    if (!slots || !ax || !ay || !az || !points)
        return fail(SDFR_EINVAL, "brick_points: null slots / axis table / points");
    int rc = grid_check("brick_points", nb);
    if (rc) return rc;
    if (slot0 >= slot1) return fail(SDFR_EINVAL, "brick_points: empty slot range");
    const uint32_t nq = nb * nb * nb, per = kSpThreads / 64;
    sp_brick_points<<<(nq + per - 1) / per, kSpThreads, 0, (hipStream_t)stream>>>(
        slots, nb, nq, slot0, slot1, ax, ay, az, points);
    return check_launch("brick_points");
}

extern "C" size_t sdfr_mc_sparse_workspace_bytes(uint32_t n_bricks) {
    if (n_bricks == 0 || 4ull * kBrick * n_bricks + 1 >= (1ull << 32)) return 0;
    return (size_t)sp_ws(n_bricks).bytes;
}

extern "C" int sdfr_mc_sparse_count(const float *values, const int32_t *slots,
                                    const uint8_t *surface, uint32_t nb, uint32_t n_bricks,
                                    float level, void *ws, size_t ws_bytes, uint8_t *grow,
                                    uint32_t *counts, void *stream) {
    SpVol m;
    SpWs w;
    int rc = sp_setup(values, slots, surface, nb, n_bricks, level, ws, ws_bytes, m, w);
    if (rc) return rc;
    if (!counts) return fail(SDFR_EINVAL, "mc_sparse: null counts");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nq = nb * nb * nb;
    uint32_t *S = (uint32_t *)ws;
    uint32_t *bsum = (uint32_t *)((char *)ws + w.bsum_off);
    uint32_t *brick_of = (uint32_t *)((char *)ws + w.brick_off);
    if (hipMemsetAsync(brick_of, 0xff, (size_t)n_bricks * sizeof(uint32_t), st) != hipSuccess ||
        (grow && hipMemsetAsync(grow, 0, nq, st) != hipSuccess))
        return fail(SDFR_ELAUNCH, "mc_sparse: clearing the tables");
    sp_brick_of<<<(nq + kSpThreads - 1) / kSpThreads, kSpThreads, 0, st>>>(slots, nq, n_bricks,
                                                                         brick_of);
    sp_classify<<<m.P / kSpThreads, kSpThreads, 0, st>>>(m, S, grow);
    exclusive_scan_u32(S, w.M, bsum, st);
    rc = check_launch("mc_sparse: count");
    if (rc) return rc;
    // counts = (vertices, triangles) = (S[3P], S[4P] - S[3P]); the subtraction on the host
    uint32_t tail[2];
    if (hipMemcpyAsync(tail, S + 3ull * m.P, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(tail + 1, S + w.M, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mc_sparse: reading the counts");
    counts[0] = tail[0];
    counts[1] = tail[1] - tail[0];
    return SDFR_OK;
}

extern "C" int sdfr_mc_sparse_emit(const float *values, const int32_t *slots,
                                   const uint8_t *surface, uint32_t nb, uint32_t n_bricks,
                                   float level, const void *ws, size_t ws_bytes, float *verts,
                                   int32_t *faces, void *stream) {
    SpVol m;
    SpWs w;
    int rc = sp_setup(values, slots, surface, nb, n_bricks, level, ws, ws_bytes, m, w);
    if (rc) return rc;
    if (!verts || !faces) return fail(SDFR_EINVAL, "mc_sparse: null verts / faces");
    sp_emit<<<m.P / kSpThreads, kSpThreads, 0, (hipStream_t)stream>>>(m, (const uint32_t *)ws,
                                                                     verts, faces);
    return check_launch("mc_sparse: emit");
}

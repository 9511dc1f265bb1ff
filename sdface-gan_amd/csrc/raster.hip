// raster.hip -- mesh rasteriser: B views of one indexed mesh, nearest triangle per pixel,
// and per-vertex attribute interpolation.  The definition (vertex projection, fixed-point
// coverage, depth, barycentrics, resolve) is pinned in include/sdfr.h, "Mesh rasteriser";
// this file is its implementation and nothing here may change a bit of it.
//
//   raster_project_kernel   one thread per (view, vertex): (X, Y, z, rz) in one 16-B store
//   raster_small_kernel     one thread per (view, face): gather, cull, clamp the bounding
//                           box; a box of <= 64 pixels is walked by the thread, one 64-bit
//                           atomic minimum per covered pixel; a larger one is appended to
//                           a list (one counter atomic per wave)
//   raster_large_kernel     a fixed grid of waves strides over that list (its length is
//                           read from device memory: no host synchronisation), the lanes
//                           of a wave stride the box's pixels
//   raster_resolve_kernel   one thread per pixel: decode the key, recompute the
//                           barycentrics, write face_idx / depth / bary
//   mesh_interpolate_kernel one thread per pixel, C channels
//
// The scatter is an integer minimum on a packed (depth bits, id) key, so no float atomics
// and no dependence on arrival order.  Keys are set to all ones beforehand (no triangle
// can produce that key: ids are < 2^31 and the depth is a positive finite float).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sdfr_common.h"

namespace sdfr {

namespace {

constexpr int kRasterThreads = 256;
constexpr int kSubpixel = 4096;           // 12 subpixel bits
constexpr int kHalf = kSubpixel / 2;
constexpr int kSmallBox = 64;             // pixels a single thread walks
constexpr int kLargeBlocks = 256;         // raster_large_kernel: 256 x 4 waves
constexpr uint32_t kMaxImage = 16384;
constexpr int32_t kBadVertex = INT32_MIN; // X of an unusable vertex

struct __attribute__((aligned(16))) ProjVertex {   // 16 B, one load / store
    int32_t X, Y;
    float z, rz;
};

struct RasterDims {
    uint32_t B, H, W, V, F;
};

__device__ __forceinline__ int32_t to_fixed(float x, bool &ok) {
    const float r = rintf(__fmul_rn(x, (float)kSubpixel));
    // (false for NaN as well)
    if (!(fabsf(r) < 1073741824.0f)) {
        ok = false;
        return 0;
    }
    return (int32_t)r;
}

__global__ void __launch_bounds__(kRasterThreads)
raster_project_kernel(const RasterDims n, const float *__restrict__ vertices,
                      const float *__restrict__ cam, const float *__restrict__ focal, float cx,
                      float cy, float znear, ProjVertex *__restrict__ proj) {
    const uint32_t t = blockIdx.x * kRasterThreads + threadIdx.x;
    if (t >= n.B * n.V) return;
    const uint32_t b = t / n.V, v = t - b * n.V;
    const float *c = cam + (size_t)b * 12;
    const float f = focal[b];
    const float d0 = __fsub_rn(vertices[(size_t)v * 3 + 0], c[3]);
    const float d1 = __fsub_rn(vertices[(size_t)v * 3 + 1], c[7]);
    const float d2 = __fsub_rn(vertices[(size_t)v * 3 + 2], c[11]);
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        q[k] = __fadd_rn(__fadd_rn(__fmul_rn(d0, c[k]), __fmul_rn(d1, c[4 + k])),
                         __fmul_rn(d2, c[8 + k]));
    const float z = -q[2];
    const float x = __fadd_rn(cx, __fdiv_rn(__fmul_rn(f, q[0]), z));
    const float y = __fsub_rn(cy, __fdiv_rn(__fmul_rn(f, q[1]), z));
    bool ok = (fabsf(z) < INFINITY) && (z > znear);
    ProjVertex p;
    p.X = to_fixed(x, ok);
    p.Y = to_fixed(y, ok);
    p.z = z;
    p.rz = __fdiv_rn(1.0f, z);
    if (!ok) p.X = kBadVertex;
    proj[t] = p;
}

struct Tri {
    int64_t Xa, Ya;
    int64_t dXb, dYb, dXc, dYc;   // (Xb - Xa), (Yb - Ya), (Xc - Xa), (Yc - Ya)
    int64_t A;                    // doubled area (signed)
    float fA;                     // float(|A|)
    float rza, rzb, rzc;
    int32_t x0, x1, y0, y1;       // clamped pixel box, inclusive; empty when x0 > x1 or y0 > y1
};

// Gather, cull and box one triangle of view b; false when it is culled whole.
__device__ __forceinline__ bool load_tri(const RasterDims &n, const int32_t *__restrict__ faces,
                                         const ProjVertex *__restrict__ proj, uint32_t b,
                                         uint32_t f, Tri &t) {
    const int32_t ia = faces[(size_t)f * 3 + 0], ib = faces[(size_t)f * 3 + 1],
                  ic = faces[(size_t)f * 3 + 2];
    if ((uint32_t)ia >= n.V || (uint32_t)ib >= n.V || (uint32_t)ic >= n.V) return false;
    const ProjVertex *pv = proj + (size_t)b * n.V;
    const ProjVertex a = pv[ia], bb = pv[ib], c = pv[ic];
    if (a.X == kBadVertex || bb.X == kBadVertex || c.X == kBadVertex) return false;
    t.Xa = a.X;
    t.Ya = a.Y;
    t.dXb = (int64_t)bb.X - a.X;
    t.dYb = (int64_t)bb.Y - a.Y;
    t.dXc = (int64_t)c.X - a.X;
    t.dYc = (int64_t)c.Y - a.Y;
    t.A = t.dXb * t.dYc - t.dYb * t.dXc;
    if (t.A == 0) return false;
    t.fA = (float)(t.A < 0 ? -t.A : t.A);
    t.rza = a.rz;
    t.rzb = bb.rz;
    t.rzc = c.rz;
    const int64_t xmin = min(a.X, min(bb.X, c.X)), xmax = max(a.X, max(bb.X, c.X));
    const int64_t ymin = min(a.Y, min(bb.Y, c.Y)), ymax = max(a.Y, max(bb.Y, c.Y));
    // pixel i can be covered only when xmin <= 4096 i + 2048 <= xmax (>> floors)
    const int64_t i0 = (xmin - kHalf + kSubpixel - 1) >> 12, i1 = (xmax - kHalf) >> 12;
    const int64_t j0 = (ymin - kHalf + kSubpixel - 1) >> 12, j1 = (ymax - kHalf) >> 12;
    t.x0 = (int32_t)max(i0, (int64_t)0);
    t.x1 = (int32_t)min(i1, (int64_t)n.W - 1);
    t.y0 = (int32_t)max(j0, (int64_t)0);
    t.y1 = (int32_t)min(j1, (int64_t)n.H - 1);
    return true;
}

// Coverage, depth and barycentrics of pixel (i, j) by the header's expressions; false
// when the pixel is not covered (or its depth is not a positive finite number).
__device__ __forceinline__ bool shade_pixel(const Tri &t, int32_t i, int32_t j, float &depth,
                                            float (&bary)[3]) {
    const int64_t px = (int64_t)i * kSubpixel + kHalf - t.Xa;
    const int64_t py = (int64_t)j * kSubpixel + kHalf - t.Ya;
    int64_t w1 = px * t.dYc - py * t.dXc;
    int64_t w2 = t.dXb * py - t.dYb * px;
    int64_t w0 = t.A - w1 - w2;
    if (t.A < 0) {
        w0 = -w0;
        w1 = -w1;
        w2 = -w2;
    }
    if ((w0 | w1 | w2) < 0) return false;
    const float l0 = __fdiv_rn((float)w0, t.fA), l1 = __fdiv_rn((float)w1, t.fA),
                l2 = __fdiv_rn((float)w2, t.fA);
    const float iz = __fadd_rn(__fadd_rn(__fmul_rn(l0, t.rza), __fmul_rn(l1, t.rzb)),
                               __fmul_rn(l2, t.rzc));
    depth = __fdiv_rn(1.0f, iz);
    if (!(depth > 0.0f && depth < INFINITY)) return false;
    bary[0] = __fmul_rn(__fmul_rn(l0, t.rza), depth);
    bary[1] = __fmul_rn(__fmul_rn(l1, t.rzb), depth);
    bary[2] = __fmul_rn(__fmul_rn(l2, t.rzc), depth);
    return true;
}

__device__ __forceinline__ void put_key(unsigned long long *__restrict__ keys,
                                        const RasterDims &n, uint32_t b, int32_t i, int32_t j,
                                        float depth, uint32_t f) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | f;
    __hip_atomic_fetch_min(keys + ((size_t)b * n.H + (uint32_t)j) * n.W + (uint32_t)i, key,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kRasterThreads)
raster_small_kernel(const RasterDims n, const int32_t *__restrict__ faces,
                    const ProjVertex *__restrict__ proj, unsigned long long *__restrict__ keys,
                    uint32_t *__restrict__ counter, uint2 *__restrict__ list) {
    const uint32_t t = blockIdx.x * kRasterThreads + threadIdx.x;
    const bool in = t < n.B * n.F;
    const uint32_t b = in ? t / n.F : 0, f = in ? t - b * n.F : 0;
    Tri tri;
    bool live = in && load_tri(n, faces, proj, b, f, tri);
    live = live && tri.x0 <= tri.x1 && tri.y0 <= tri.y1;
    bool big = false;
    if (live) {
        const uint32_t bw = (uint32_t)(tri.x1 - tri.x0 + 1), bh = (uint32_t)(tri.y1 - tri.y0 + 1);
        big = (uint64_t)bw * bh > (uint64_t)kSmallBox;
        if (!big) {
            for (int32_t j = tri.y0; j <= tri.y1; ++j)
                for (int32_t i = tri.x0; i <= tri.x1; ++i) {
                    float depth, bary[3];
                    if (shade_pixel(tri, i, j, depth, bary)) put_key(keys, n, b, i, j, depth, f);
                }
        }
    }
    // large boxes: one counter atomic per wave, the wave's entries are consecutive
    // (every lane of the wave reaches this point: nothing above returns)
    const unsigned long long m = __ballot(big);
    if (m) {
        const uint32_t lane = __lane_id();
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (big) {
            const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (slot < n.B * n.F) list[slot] = make_uint2(b, f);
        }
    }
}

__global__ void __launch_bounds__(kRasterThreads)
raster_large_kernel(const RasterDims n, const int32_t *__restrict__ faces,
                    const ProjVertex *__restrict__ proj, unsigned long long *__restrict__ keys,
                    const uint32_t *__restrict__ counter, const uint2 *__restrict__ list) {
    const uint32_t count = min(*counter, n.B * n.F);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * kRasterThreads + threadIdx.x) >> 6;
    const uint32_t waves = (gridDim.x * kRasterThreads) >> 6;
    for (uint32_t e = wave; e < count; e += waves) {
        const uint2 bf = list[e];
        if (bf.x >= n.B || bf.y >= n.F) continue;
        Tri tri;
        if (!load_tri(n, faces, proj, bf.x, bf.y, tri)) continue;
        if (tri.x0 > tri.x1 || tri.y0 > tri.y1) continue;
        const uint32_t bw = (uint32_t)(tri.x1 - tri.x0 + 1), bh = (uint32_t)(tri.y1 - tri.y0 + 1);
        const uint32_t npix = bw * bh;            // <= 16384^2
        for (uint32_t p = lane; p < npix; p += 64u) {
            const uint32_t r = p / bw;
            const int32_t i = tri.x0 + (int32_t)(p - r * bw), j = tri.y0 + (int32_t)r;
            float depth, bary[3];
            if (shade_pixel(tri, i, j, depth, bary)) put_key(keys, n, bf.x, i, j, depth, bf.y);
        }
    }
}

__global__ void __launch_bounds__(kRasterThreads)
raster_resolve_kernel(const RasterDims n, const int32_t *__restrict__ faces,
                      const ProjVertex *__restrict__ proj,
                      const unsigned long long *__restrict__ keys, int32_t *__restrict__ face_idx,
                      float *__restrict__ depth_out, float *__restrict__ bary_out) {
    const uint32_t t = blockIdx.x * kRasterThreads + threadIdx.x;
    if (t >= n.B * n.H * n.W) return;
    const uint32_t i = t % n.W, r = t / n.W, j = r % n.H, b = r / n.H;
    const unsigned long long key = keys[t];
    int32_t id = -1;
    float depth = 0.0f, bary[3] = {0.0f, 0.0f, 0.0f};
    if (key != ~0ull) {
        const uint32_t f = (uint32_t)(key & 0xffffffffull);
        Tri tri;
        // (the key was written for this pixel by this triangle: both hold again)
        if (f < n.F && load_tri(n, faces, proj, b, f, tri) &&
            shade_pixel(tri, (int32_t)i, (int32_t)j, depth, bary)) {
            id = (int32_t)f;
        } else {
            depth = 0.0f;
            bary[0] = bary[1] = bary[2] = 0.0f;
        }
    }
    if (face_idx) face_idx[t] = id;
    if (depth_out) depth_out[t] = depth;
    if (bary_out) {
        bary_out[(size_t)t * 3 + 0] = bary[0];
        bary_out[(size_t)t * 3 + 1] = bary[1];
        bary_out[(size_t)t * 3 + 2] = bary[2];
    }
}

__global__ void __launch_bounds__(kRasterThreads)
mesh_interpolate_kernel(const float *__restrict__ attr, uint32_t V, uint32_t C,
                        const int32_t *__restrict__ faces, uint32_t F,
                        const int32_t *__restrict__ face_idx, const float *__restrict__ bary,
                        uint32_t B, uint32_t HW, const float *__restrict__ background,
                        uint32_t background_batch, float fill, float *__restrict__ out) {
    const uint32_t t = blockIdx.x * kRasterThreads + threadIdx.x;
    if (t >= B * HW) return;
    const uint32_t b = t / HW, p = t - b * HW;
    const int32_t f = face_idx[t];
    int32_t i0 = 0, i1 = 0, i2 = 0;
    bool covered = (uint32_t)f < F;
    if (covered) {
        i0 = faces[(size_t)f * 3 + 0];
        i1 = faces[(size_t)f * 3 + 1];
        i2 = faces[(size_t)f * 3 + 2];
        covered = (uint32_t)i0 < V && (uint32_t)i1 < V && (uint32_t)i2 < V;
    }
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
    if (covered) {
        w0 = bary[(size_t)t * 3 + 0];
        w1 = bary[(size_t)t * 3 + 1];
        w2 = bary[(size_t)t * 3 + 2];
    }
    const uint32_t bb = background_batch == 1 ? 0u : b;
    for (uint32_t c = 0; c < C; ++c) {
        float v;
        if (covered) {
            v = __fadd_rn(__fadd_rn(__fmul_rn(w0, attr[(size_t)i0 * C + c]),
                                    __fmul_rn(w1, attr[(size_t)i1 * C + c])),
                          __fmul_rn(w2, attr[(size_t)i2 * C + c]));
        } else {
            v = background ? background[((size_t)bb * C + c) * HW + p] : fill;
        }
        out[((size_t)b * C + c) * HW + p] = v;
    }
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

bool raster_sizes_ok(uint32_t B, uint32_t H, uint32_t W, uint32_t V, uint32_t F) {
    if (!B || !H || !W || !V || !F) return false;
    if (H > kMaxImage || W > kMaxImage) return false;
    const uint64_t lim = 1ull << 31;
    return (uint64_t)B * V < lim && (uint64_t)B * F < lim && (uint64_t)B * H * W < lim;
}

inline uint32_t blocks_for(uint64_t threads) {
    return (uint32_t)((threads + kRasterThreads - 1) / kRasterThreads);
}

}  // namespace

}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_mesh_raster_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t V,
                                                   uint32_t F) {
    if (!raster_sizes_ok(B, H, W, V, F)) return 0;
    return up256((size_t)B * V * sizeof(ProjVertex)) + up256((size_t)B * H * W * 8) + 256 +
           up256((size_t)B * F * sizeof(uint2));
}

extern "C" int sdfr_mesh_raster(const sdfr_raster_args *a, void *stream) {
    if (!a) return fail(SDFR_EINVAL, "mesh_raster: null arguments");
    if (!raster_sizes_ok(a->B, a->H, a->W, a->V, a->F))
        return fail(SDFR_EINVAL, "mesh_raster: sizes must be nonzero, H and W <= 16384, "
                                 "B V, B F and B H W < 2^31");
    if (!a->vertices || !a->faces || !a->cam || !a->focal)
        return fail(SDFR_EINVAL, "mesh_raster: null vertices / faces / cam / focal");
    if (!a->face_idx && !a->depth && !a->bary)
        return fail(SDFR_EINVAL, "mesh_raster: every output is null");
    if (!(a->znear >= 0.0f) || !std::isfinite(a->znear) || !std::isfinite(a->cx) ||
        !std::isfinite(a->cy))
        return fail(SDFR_EINVAL, "mesh_raster: znear must be finite and >= 0, cx and cy finite");
    if (!a->workspace ||
        a->workspace_bytes < sdfr_mesh_raster_workspace_bytes(a->B, a->H, a->W, a->V, a->F))
        return fail(SDFR_EINVAL, "mesh_raster: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const RasterDims n{a->B, a->H, a->W, a->V, a->F};
    char *ws = (char *)a->workspace;
    ProjVertex *proj = (ProjVertex *)ws;
    ws += up256((size_t)n.B * n.V * sizeof(ProjVertex));
    unsigned long long *keys = (unsigned long long *)ws;
    const size_t key_bytes = (size_t)n.B * n.H * n.W * 8;
    ws += up256(key_bytes);
    uint32_t *counter = (uint32_t *)ws;
    ws += 256;
    uint2 *list = (uint2 *)ws;
    if (hipMemsetAsync(keys, 0xff, key_bytes, st) != hipSuccess ||
        hipMemsetAsync(counter, 0, 256, st) != hipSuccess)
        return fail(SDFR_ELAUNCH, "mesh_raster: clearing the keys");
    raster_project_kernel<<<blocks_for((uint64_t)n.B * n.V), kRasterThreads, 0, st>>>(
        n, a->vertices, a->cam, a->focal, a->cx, a->cy, a->znear, proj);
    raster_small_kernel<<<blocks_for((uint64_t)n.B * n.F), kRasterThreads, 0, st>>>(
        n, a->faces, proj, keys, counter, list);
    raster_large_kernel<<<kLargeBlocks, kRasterThreads, 0, st>>>(n, a->faces, proj, keys, counter,
                                                                 list);
    raster_resolve_kernel<<<blocks_for((uint64_t)n.B * n.H * n.W), kRasterThreads, 0, st>>>(
        n, a->faces, proj, keys, a->face_idx, a->depth, a->bary);
    return check_launch("mesh_raster");
}

extern "C" int sdfr_mesh_interpolate(const float *attr, uint32_t V, uint32_t C,
                                     const int32_t *faces, uint32_t F, const int32_t *face_idx,
                                     const float *bary, uint32_t B, uint32_t H, uint32_t W,
                                     const float *background, uint32_t background_batch,
                                     float fill, float *out, void *stream) {
    if (!attr || !faces || !face_idx || !bary || !out)
        return fail(SDFR_EINVAL, "mesh_interpolate: null attr / faces / face_idx / bary / out");
    if (!V || !C || !F || !B || !H || !W)
        return fail(SDFR_EINVAL, "mesh_interpolate: zero size");
    if (background && background_batch != 1 && background_batch != B)
        return fail(SDFR_EINVAL, "mesh_interpolate: background_batch must be 1 or B");
    if ((uint64_t)B * C * H * W >= (1ull << 31) || (uint64_t)V * C >= (1ull << 31))
        return fail(SDFR_EINVAL, "mesh_interpolate: B C H W and V C must be < 2^31");
    mesh_interpolate_kernel<<<blocks_for((uint64_t)B * H * W), kRasterThreads, 0,
                              (hipStream_t)stream>>>(attr, V, C, faces, F, face_idx, bary, B,
                                                     H * W, background, background_batch, fill,
                                                     out);
    return check_launch("mesh_interpolate");
}

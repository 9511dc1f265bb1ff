// surface.hip -- the ray-side kernels of the surface render (sdfr_render_ngp_surface,
// sdfr_render_siren_surface; entry points in render_api.hip): per camera ray the first
// outside -> inside sign change of the SDF among the render's samples, refined by a fixed
// number of bisection steps, and the maps at that point.  Every SDF, gradient and colour
// value comes from the query and gradient calls' kernels, unchanged; the kernels here only
// move per-ray state between those calls.
//
//   geom_points_kernel   the render's samples as points, plain [B,H,W,N] order (geometry.hip)
//   surf_bracket_kernel  sdf [rays][N] -> per ray s* (the smallest s with sdf_s > 0 and
//                        sdf_{s+1} <= 0, or -1) and the bracket (a, b, fa, fb)
//   surf_step_kernel     one bisection step: narrow the bracket with the previous
//                        midpoint's SDF, write the next midpoint's network coordinate
//   surf_hit_kernel      the last narrowing, the linear interpolation z*, the hit point's
//                        network coordinate and the ray's view direction
//   surf_maps_kernel     the maps [B,C,H,W] from z*, the gradient call's output and the
//                        colour query's
//
// Every expression on z and on a point is one rounded operation per step of the definition
// (include/sdfr.h), with geom_points_kernel's ops for a point, so a caller can reproduce the
// result bit for bit from the query call.
//
// Thread mapping.  The coarse SDF is sample-major per ray (index ray N + s), everything else
// is per ray.  surf_bracket_kernel reads the SDF in memory order: a wave owns 64 / N
// consecutive rays (one when N > 32), lane l holds sample l % N of ray l / N, so a wave load
// is one contiguous run of dwords; one thread per ray would touch 64 cache lines per wave
// load (geometry.hip).  The s + 1 neighbour comes from lane l + 1; the crossing test is one
// wave ballot, and each ray takes the first set bit of its own N-lane segment.  A ray of
// N > 64 samples takes chunks of 64 lanes in order and stops at the first chunk with a set
// bit; lane 63's neighbour, the next chunk's first sample, is the one value read from memory
// a second time, which is how a crossing between samples 64 c + 63 and 64 c + 64 is found.
// The other kernels are one thread per ray (or per padded refinement point): 16-B and 4-B
// loads and stores at consecutive addresses, the ray rebuilt from the camera (~30 flops).
#include "render_launch.h"
#include "render_ngp.h"

namespace sdfr {

namespace {

// face b's ray rl (y W + x) of the call
__device__ __forceinline__ void surf_ray(const GeomArgs &g, uint32_t b, uint32_t rl, Ray &r) {
    make_ray(g.cam + (size_t)b * 12, g.focal[b], g.pix_x[rl % g.W], g.pix_y[rl / g.W], g.half_res,
             r);
}

// p = fadd(o, fmul(d, z)) and its network coordinate (geom_points_kernel's ops)
__device__ __forceinline__ void surf_point(const GeomArgs &g, const Ray &r, uint32_t b, float z,
                                           float (&p)[3], float (&pn)[3]) {
    const float span = __fsub_rn(g.far_[b], g.near_[b]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = __fadd_rn(r.o[k], __fmul_rn(r.d[k], z));
        pn[k] = g.z_normalize ? __fdiv_rn(__fmul_rn(p[k], 2.0f), span) : p[k];
    }
}

__device__ __forceinline__ float surf_mid(const f4 &br) {
    return __fmul_rn(0.5f, __fadd_rn(br.x, br.y));
}

// the bracket (a, b, fa, fb) after the SDF f at its midpoint: f > 0 moves a, else b
__device__ __forceinline__ void surf_narrow(f4 &br, float f) {
    const float m = surf_mid(br);
    if (f > 0.0f) {
        br.x = m;
        br.z = f;
    } else {
        br.y = m;
        br.w = f;
    }
}

}  // namespace

constexpr uint32_t kBracketWaves = 4;

__global__ void __launch_bounds__(kBracketWaves * 64)
surf_bracket_kernel(const float *__restrict__ sdf, const float2 *__restrict__ zd, uint32_t rays,
                    uint32_t N, uint32_t rpw, f4 *__restrict__ br, int32_t *__restrict__ sidx) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * kBracketWaves + (threadIdx.x >> 6);
    const uint32_t ray0 = wave * rpw;                       // wave-uniform
    if (ray0 >= rays) return;
    // lane -> (ray of the wave, sample of the chunk); N > 32: one ray, 64 samples a chunk
    const uint32_t rw = rpw > 1 ? lane / N : 0u, sl = rpw > 1 ? lane % N : lane;
    const uint32_t ray = ray0 + rw;
    const bool ray_ok = rw < rpw && ray < rays;
    const uint32_t nchunk = rpw > 1 ? 1u : (N + 63u) / 64u;
    uint64_t found = 0;
    uint32_t c = 0;
    for (; c < nchunk; ++c) {
        const uint32_t s = c * 64u + sl;
        const bool have = ray_ok && s < N, next = ray_ok && s + 1 < N;
        const size_t idx = (size_t)ray * N + s;
        const float v = have ? sdf[idx] : 0.0f;
        float vn = __shfl_down(v, 1);                       // every lane takes part
        if (lane == 63u && next) vn = sdf[idx + 1];         // the next chunk's first sample
        found = __ballot(next && v > 0.0f && vn <= 0.0f);   // NaN: neither holds
        if (found) break;                                   // wave-uniform
    }
    // lane j stores ray j of the wave: the first set bit of that ray's N-lane segment
    if (lane >= rpw || ray0 + lane >= rays) return;
    const uint32_t r = ray0 + lane;
    const uint64_t seg = rpw > 1 ? (found >> (lane * N)) & ((1ull << N) - 1ull) : found;
    const size_t base = (size_t)r * N;
    if (seg == 0) {
        // a miss: a valid bracket at the first sample, which the later kernels ignore
        const float z0 = zd[base].x;
        br[r] = f4{z0, z0, 0.0f, 0.0f};
        sidx[r] = -1;
        return;
    }
    const uint32_t s = c * 64u + (uint32_t)__ffsll((unsigned long long)seg) - 1u;
    br[r] = f4{zd[base + s].x, zd[base + s + 1].x, sdf[base + s], sdf[base + s + 1]};
    sidx[r] = (int32_t)s;
}

// One bisection step over the padded refinement points: face b's point i < HW is its ray i,
// the points up to Mp (HW rounded up to the query's group of 32) are padding and get the
// origin once.  f: the SDF at the previous midpoints [B][Mp], or null on the first step.
__global__ void __launch_bounds__(256)
surf_step_kernel(const GeomArgs g, uint32_t Mp, uint32_t total, const float *__restrict__ f,
                 f4 *__restrict__ br, float *__restrict__ pts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t HW = g.H * g.W, b = i / Mp, rl = i % Mp;
    float pn[3] = {0.0f, 0.0f, 0.0f};
    if (rl < HW) {
        const uint32_t ray = b * HW + rl;
        f4 v = br[ray];
        if (f) {
            surf_narrow(v, f[i]);
            br[ray] = v;
        }
        Ray r;
        surf_ray(g, b, rl, r);
        float p[3];
        surf_point(g, r, b, surf_mid(v), p, pn);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) pts[(size_t)i * 3 + k] = pn[k];
}

// The last narrowing (f non-null), then z* = a + fa / (fa - fb) (b - a) clamped to [a, b]
// (fa > 0 >= fb: the divisor is positive), the hit point's network coordinate [rays][3] and
// the direction the render gives the network for the ray [rays][3].  A miss keeps its
// placeholder bracket: a valid point, ignored by surf_maps_kernel.
__global__ void __launch_bounds__(256)
surf_hit_kernel(const GeomArgs g, uint32_t Mp, uint32_t rays, const float *__restrict__ f,
                const f4 *__restrict__ br, const int32_t *__restrict__ sidx,
                float *__restrict__ zs, float *__restrict__ pnet, float *__restrict__ dirs) {
    const uint32_t ray = blockIdx.x * 256 + threadIdx.x;
    if (ray >= rays) return;
    const uint32_t HW = g.H * g.W, b = ray / HW, rl = ray % HW;
    f4 v = br[ray];
    if (f) surf_narrow(v, f[(size_t)b * Mp + rl]);
    float z = v.x;
    if (sidx[ray] >= 0) {
        const float t = __fdiv_rn(v.z, __fsub_rn(v.z, v.w));
        z = __fadd_rn(v.x, __fmul_rn(t, __fsub_rn(v.y, v.x)));
        z = fminf(fmaxf(z, v.x), v.y);
    }
    zs[ray] = z;
    Ray r;
    surf_ray(g, b, rl, r);
    float p[3], pn[3];
    surf_point(g, r, b, z, p, pn);
    const float v0 = g.static_viewdirs ? r.dir[0] : r.d[0];
    const float v1 = g.static_viewdirs ? r.dir[1] : r.d[1];
    const float v2 = g.static_viewdirs ? r.dir[2] : r.d[2];
    const float vn = norm3_torch(v0, v1, v2);
    const float u[3] = {__fdiv_rn(v0, vn), __fdiv_rn(v1, vn), __fdiv_rn(v2, vn)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pnet[(size_t)ray * 3 + k] = pn[k];
        dirs[(size_t)ray * 3 + k] = u[k];
    }
}

struct SurfMapArgs {
    GeomArgs g;
    uint32_t rays;
    const int32_t *sidx;           // [rays]
    const float *zs;               // [rays] z*
    const float *gsdf, *ggrad;     // [rays], [rays][3] the gradient call at the hit points
    const float *rgbq;             // [rays][3] the colour query there
    float *hit, *depth, *residual, *xyz, *normal, *rgb;   // each may be null
    int32_t *sample;
};

__global__ void __launch_bounds__(256) surf_maps_kernel(const SurfMapArgs a) {
    const uint32_t ray = blockIdx.x * 256 + threadIdx.x;
    if (ray >= a.rays) return;
    const GeomArgs &G = a.g;
    const uint32_t HW = G.H * G.W, b = ray / HW, pix = ray % HW;
    const int32_t s = a.sidx[ray];
    const bool hit = s >= 0;
    if (a.hit) a.hit[ray] = hit ? 1.0f : 0.0f;
    if (a.sample) a.sample[ray] = s;
    const float z = a.zs[ray];
    if (a.depth) a.depth[ray] = hit ? z : 0.0f;
    if (a.residual) a.residual[ray] = hit ? a.gsdf[ray] : 0.0f;
    if (a.xyz) {
        Ray r;
        surf_ray(G, b, pix, r);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            a.xyz[((size_t)b * 3 + k) * HW + pix] =
                hit ? __fadd_rn(r.o[k], __fmul_rn(r.d[k], z)) : 0.0f;
    }
    if (a.normal) {
        // the geometry render's eikonal formula, then e / max(|e|, 1e-20)
        float e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = a.ggrad[(size_t)ray * 3 + k];
        if (G.z_normalize) {
            const float span = __fsub_rn(G.far_[b], G.near_[b]);
#pragma unroll
            for (int k = 0; k < 3; ++k) e[k] = __fdiv_rn(__fmul_rn(e[k], 2.0f), span);
        }
        const float len = fmaxf(norm3_torch(e[0], e[1], e[2]), 1e-20f);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            a.normal[((size_t)b * 3 + k) * HW + pix] = hit ? __fdiv_rn(e[k], len) : 0.0f;
    }
    if (a.rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            a.rgb[((size_t)b * 3 + k) * HW + pix] = hit ? a.rgbq[(size_t)ray * 3 + k] : 0.0f;
    }
}

int launch_surf_bracket(const GeomArgs &g, const float *sdf, const float2 *zd, f4 *br,
                        int32_t *sidx, hipStream_t st) {
    const uint32_t rays = g.B * g.H * g.W;
    const uint32_t rpw = g.N > 32 ? 1u : 64u / g.N;         // rays per wave
    const uint32_t waves = (rays + rpw - 1) / rpw;
    hipLaunchKernelGGL(surf_bracket_kernel, dim3((waves + kBracketWaves - 1) / kBracketWaves),
                       dim3(kBracketWaves * 64), 0, st, sdf, zd, rays, g.N, rpw, br, sidx);
    return check_launch("render_surface: bracket");
}

int launch_surf_step(const GeomArgs &g, uint32_t Mp, const float *f, f4 *br, float *pts,
                     hipStream_t st) {
    const uint32_t total = g.B * Mp;
    hipLaunchKernelGGL(surf_step_kernel, dim3((total + 255) / 256), dim3(256), 0, st, g, Mp, total,
                       f, br, pts);
    return check_launch("render_surface: bisection step");
}

int launch_surf_hit(const GeomArgs &g, uint32_t Mp, const float *f, const f4 *br,
                    const int32_t *sidx, float *zs, float *pnet, float *dirs, hipStream_t st) {
    const uint32_t rays = g.B * g.H * g.W;
    hipLaunchKernelGGL(surf_hit_kernel, dim3((rays + 255) / 256), dim3(256), 0, st, g, Mp, rays, f,
                       br, sidx, zs, pnet, dirs);
    return check_launch("render_surface: hit points");
}

int launch_surf_maps(const GeomArgs &g, const int32_t *sidx, const float *zs, const float *gsdf,
                     const float *ggrad, const float *rgbq, float *hit, int32_t *sample,
                     float *depth, float *residual, float *xyz, float *normal, float *rgb,
                     hipStream_t st) {
    SurfMapArgs a;
    a.g = g;
    a.rays = g.B * g.H * g.W;
    a.sidx = sidx;
    a.zs = zs;
    a.gsdf = gsdf;
    a.ggrad = ggrad;
    a.rgbq = rgbq;
    a.hit = hit;
    a.sample = sample;
    a.depth = depth;
    a.residual = residual;
    a.xyz = xyz;
    a.normal = normal;
    a.rgb = rgb;
    hipLaunchKernelGGL(surf_maps_kernel, dim3((a.rays + 255) / 256), dim3(256), 0, st, a);
    return check_launch("render_surface: maps");
}

}  // namespace sdfr

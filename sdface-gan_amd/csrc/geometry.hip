// geometry.hip -- the render-time use of the fused SDF gradient (sdfr_render_ngp_geometry,
// entry point in render_api.hip): the camera rays' samples go through the gradient call's
// kernels, and a compositing kernel turns the per-sample SDF and gradient into maps.
//
//   geom_points_kernel       cameras -> per sample the network coordinate p_net (what the
//                            gradient gather reads as `points`) and (z, dist), in plain
//                            [B,H,W,N] order: point (y W + x) N + s of its face
//   ngp_encode_grad_kernel,
//   field_g_kernel           the gradient call's gather and field kernel, unchanged
//                            (field_grad.hip), on B x (H W N) points
//   geom_composite_kernel    eikonal = d sdf / d world point per sample; the render's
//                            compositing weights front to back in fp32; normal, depth, xyz
//                            and mask composited with them
//
// geom_points_kernel uses the rounded operations of sample_geom_kernel (render_ngp.hip):
// p = fadd(o, fmul(d, z)), p_net = fdiv(fmul(p, 2), far - near) under z_normalize; the
// gather forms u from p_net with its own three rounded ops -- together the render's ops, so
// the SDF of this path equals the render's return_sdf output bit for bit.
//
// Thread mapping.  The per-sample arrays are sample-major per ray (index ray N + s), the
// maps are ray-major.  geom_points_kernel is one thread per sample: consecutive lanes store
// consecutive samples (the ray is rebuilt per sample: ~30 flops against a 20-B store).
// geom_composite_kernel runs a workgroup on R consecutive rays in two phases per chunk of C
// samples (R (C|1) <= kCompSamples; C = N up to 2047 samples per ray): phase 1 walks the
// chunk's R x C samples in memory order, one sample per thread and step -- coalesced loads
// of sdf / (z, dist) / g_net, the coalesced eikonal store -- and leaves alpha, z and the
// eikonal vector in LDS at an odd row stride (conflict-free column reads); phase 2 is one
// thread per ray, front to back over the chunk from LDS, the transmittance and the
// accumulators carried in registers across chunks.  The map stores are one ray per lane.
// One thread per ray reading global memory directly would touch 64 cache lines per wave
// load (stride 4 N bytes).
#include "render_launch.h"
#include "render_ngp.h"

namespace sdfr {

__global__ void __launch_bounds__(256) geom_points_kernel(const GeomArgs g, uint32_t S,
                                                          float *__restrict__ pnet,
                                                          float2 *__restrict__ zd) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const uint32_t ray = i / g.N, s = i % g.N;
    const uint32_t HW = g.H * g.W;
    const uint32_t b = ray / HW, rl = ray % HW;
    const uint32_t y = rl / g.W, x = rl % g.W;
    Ray r;
    make_ray(g.cam + (size_t)b * 12, g.focal[b], g.pix_x[x], g.pix_y[y], g.half_res, r);
    const float nr = g.near_[b], fr = g.far_[b];
    const float span = __fsub_rn(fr, nr);
    const float dnorm = norm3_torch(r.d[0], r.d[1], r.d[2]);
    const float z = sample_z(g.sc, nr, fr, ray, s);
    const float dist = s + 1 < g.N
                           ? __fmul_rn(__fsub_rn(sample_z(g.sc, nr, fr, ray, s + 1), z), dnorm)
                           : __fmul_rn(1e10f, dnorm);
    zd[i] = make_float2(z, dist);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = __fadd_rn(r.o[k], __fmul_rn(r.d[k], z));                       // :343
        pnet[(size_t)i * 3 + k] = g.z_normalize ? __fdiv_rn(__fmul_rn(p, 2.0f), span) : p;  // :349
    }
}

constexpr uint32_t kCompSamples = 2048;      // samples of a workgroup's chunk held in LDS

struct CompArgs {
    GeomArgs g;
    uint32_t rays;                 // B H W
    uint32_t R, C;                 // rays per workgroup, samples per chunk
    const float2 *zd;              // [rays N] (z, dist)
    const float *sdf;              // [rays N]
    const float *gnet;             // [rays N][3] d sdf / d p_net
    const float *sigmoid_beta;
    int force_background;
    float *eikonal, *normal, *depth, *xyz, *mask;   // each may be null
};

__global__ void __launch_bounds__(256) geom_composite_kernel(const CompArgs a) {
    __shared__ float l_alpha[kCompSamples], l_z[kCompSamples], l_e[3][kCompSamples];
    const GeomArgs &G = a.g;
    const uint32_t N = G.N, HW = G.H * G.W;
    const uint32_t ray0 = blockIdx.x * a.R;
    const uint32_t Cs = a.C | 1u;                       // odd LDS row stride
    const bool maps = a.normal || a.depth || a.xyz || a.mask;
    const float beta = a.sigmoid_beta[0];

    // phase 2 state: this thread's ray
    const uint32_t my = ray0 + threadIdx.x;
    const bool mine = maps && threadIdx.x < a.R && my < a.rays;
    Ray ray;
    if (mine && a.xyz) {
        const uint32_t b = my / HW, rl = my % HW;
        make_ray(G.cam + (size_t)b * 12, G.focal[b], G.pix_x[rl % G.W], G.pix_y[rl / G.W],
                 G.half_res, ray);
    }
    float T = 1.0f, wsum = 0.0f, w_last = 0.0f, dacc = 0.0f;
    float nacc[3] = {0.0f, 0.0f, 0.0f}, xacc[3] = {0.0f, 0.0f, 0.0f};

    for (uint32_t c0 = 0; c0 < N; c0 += a.C) {
        const uint32_t cn = min(a.C, N - c0);           // samples of this chunk
        // phase 1: the chunk's samples in memory order
        for (uint32_t i = threadIdx.x; i < a.R * cn; i += 256) {
            const uint32_t r = i / cn, c = i % cn;
            const uint32_t rr = ray0 + r;
            if (rr >= a.rays) break;                    // r grows with i
            const uint32_t idx = rr * N + c0 + c;
            const uint32_t b = rr / HW;
            float e[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) e[k] = a.gnet[(size_t)idx * 3 + k];
            if (G.z_normalize) {
                // chain rule of normalized_pts = pts * 2 / (far - near)
                const float span = __fsub_rn(G.far_[b], G.near_[b]);
#pragma unroll
                for (int k = 0; k < 3; ++k) e[k] = __fdiv_rn(__fmul_rn(e[k], 2.0f), span);
            }
            if (a.eikonal) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.eikonal[(size_t)idx * 3 + k] = e[k];
            }
            if (maps) {
                const float2 v = a.zd[idx];
                const float sdf = a.sdf[idx];
                // volume_integration (sdf_model.py:236-301)
                const float sig = __fdiv_rn(sigmoidf_(__fdiv_rn(-sdf, beta)), beta);
                const uint32_t o = r * Cs + c;
                l_alpha[o] = 1.0f - expf(-sig * v.y);
                l_z[o] = v.x;
#pragma unroll
                for (int k = 0; k < 3; ++k) l_e[k][o] = e[k];
            }
        }
        if (!maps) continue;                            // uniform: no barrier needed
        __syncthreads();
        // phase 2: one thread per ray, front to back
        if (mine) {
            for (uint32_t c = 0; c < cn; ++c) {
                const uint32_t o = threadIdx.x * Cs + c;
                const float alpha = l_alpha[o], z = l_z[o];
                float w = alpha * T;
                if (a.force_background && c0 + c + 1 == N) w = 1.0f - wsum;
                T = T * ((1.0f - alpha) + 1e-10f);
                wsum += w;
                w_last = w;
                dacc = __fmaf_rn(w, z, dacc);
#pragma unroll
                for (int k = 0; k < 3; ++k) nacc[k] = __fmaf_rn(w, l_e[k][o], nacc[k]);
                if (a.xyz) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        xacc[k] = __fmaf_rn(w, __fadd_rn(ray.o[k], __fmul_rn(ray.d[k], z)), xacc[k]);
                }
            }
        }
        __syncthreads();                                // LDS is rewritten by the next chunk
    }
    if (!mine) return;
    const uint32_t b = my / HW, pix = my % HW;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (a.normal) a.normal[((size_t)b * 3 + k) * HW + pix] = nacc[k];
        if (a.xyz) a.xyz[((size_t)b * 3 + k) * HW + pix] = xacc[k];
    }
    if (a.depth) a.depth[(size_t)b * HW + pix] = dacc;
    if (a.mask) a.mask[(size_t)b * HW + pix] = w_last;
}

int launch_geom_points(const GeomArgs &g, float *pnet, float2 *zd, hipStream_t st) {
    const uint32_t S = g.B * g.H * g.W * g.N;           // < 2^25 (host check)
    hipLaunchKernelGGL(geom_points_kernel, dim3((S + 255) / 256), dim3(256), 0, st, g, S, pnet, zd);
    return check_launch("render_ngp_geometry: sample points");
}

int launch_geom_composite(const GeomArgs &g, const float2 *zd, const float *sdf,
                          const float *gnet, const float *sigmoid_beta, int force_background,
                          float *eikonal, float *normal, float *depth, float *xyz, float *mask,
                          hipStream_t st) {
    CompArgs a;
    a.g = g;
    a.rays = g.B * g.H * g.W;
    a.C = g.N < kCompSamples ? g.N : kCompSamples - 1;
    const uint32_t fit = kCompSamples / (a.C | 1u);
    a.R = fit < 256u ? fit : 256u;
    a.zd = zd;
    a.sdf = sdf;
    a.gnet = gnet;
    a.sigmoid_beta = sigmoid_beta;
    a.force_background = force_background;
    a.eikonal = eikonal;
    a.normal = normal;
    a.depth = depth;
    a.xyz = xyz;
    a.mask = mask;
    hipLaunchKernelGGL(geom_composite_kernel, dim3((a.rays + a.R - 1) / a.R), dim3(256), 0, st, a);
    return check_launch("render_ngp_geometry: composite");
}

}  // namespace sdfr

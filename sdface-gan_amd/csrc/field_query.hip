// field_query.hip -- the fused field evaluated at caller-supplied points
// (sdfr_query_ngp_forward, sdfr_query_siren_forward; entry points in render_api.hip):
//
//   query_geom_kernel            points [B,R,N,3] -> gu [S] (grid coordinate, inside flag)
//                                in the render's tile order with H = 1, W = R
//   ngp_encode_kernel            the render's hash-grid gather, unchanged (render_ngp.hip)
//   field_r_kernel<NgpQueryNet>  the render's split-fp16 MLP with the group's direction
//                                read from memory, no compositing, and a per-sample
//                                store of the SDF and the colour
//
// The field kernel is the template of field_r.h, instantiated HERE and nowhere
// else: co-compiled instantiations of one kernel template share register-allocation
// context, so a query instantiation beside the render's would move the render kernels'
// code.  This unit is built with field_f16x3.hip's flags.
//
// The SIREN query is field_p_kernel<SirenQueryNet>, at the end of this file: the render's
// wave-pair kernel with the point and the group's direction read from memory.  It has no
// gather and no staging kernel.  field_r_kernel<NgpQueryNet> comes out of the compiler
// unchanged beside it (profiles/siren_query_isa.txt).
#include "field_p.h"
#include "field_r.h"

namespace sdfr {

// One workgroup: one 16-group tile x up to 16 consecutive points of each group.  The
// chunk's coordinates are loaded in memory order (a group's points are contiguous, so
// consecutive lanes read consecutive dwords of runs of 3 cs floats; the whole tile is one
// run when N <= 16) into LDS, then each thread forms one point's u and stores it as one
// 16-B value in tile order (sample-major, group fastest: 256 consecutive f4).  u uses the
// rounded ops of the render's sample_geom_kernel (grid.py:149); the points are already
// network coordinates, so its z-normalisation step (sdf_model.py:349) is the caller's.
__global__ void __launch_bounds__(256) query_geom_kernel(const float *__restrict__ points,
                                                         f4 *__restrict__ gu, uint32_t R,
                                                         uint32_t N, uint32_t tiles_per_face,
                                                         uint32_t nchunk, float bound) {
    __shared__ float pl[kTileRays * 16 * 3];
    const uint32_t tile = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
    const uint32_t b = tile / tiles_per_face;
    const uint32_t r0 = (tile % tiles_per_face) * kTileRays;   // first group of the tile
    const uint32_t s0 = chunk * 16, cs = min(16u, N - s0);     // samples [s0, s0 + cs)
    const uint32_t run = 3 * cs;
    for (uint32_t i = threadIdx.x; i < kTileRays * run; i += 256) {
        const uint32_t n = i / run, off = i % run;
        if (r0 + n < R)
            pl[i] = points[(((size_t)b * R + r0 + n) * N + s0) * 3 + off];
    }
    __syncthreads();
    const uint32_t n = threadIdx.x & 15u, sl = threadIdx.x >> 4;
    if (sl >= cs) return;
    f4 u = {0.0f, 0.0f, 0.0f, 0.0f};                            // padding groups: flag 0
    if (r0 + n < R) {
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float p = pl[n * run + sl * 3 + k];
            u[k] = __fdiv_rn(__fadd_rn(p, bound), __fmul_rn(2.0f, bound));   // grid.py:149
            if (u[k] < 0 || u[k] > 1) in = false;
        }
        u[3] = in ? 1.0f : 0.0f;
    }
    gu[((size_t)tile * N + s0 + sl) * kTileRays + n] = u;
}

int launch_query_geom(const float *points, f4 *gu, const GeomArgs &g, hipStream_t st) {
    const uint32_t nchunk = (g.N + 15) / 16;
    hipLaunchKernelGGL(query_geom_kernel, dim3(g.total_tiles * nchunk), dim3(256), 0, st, points,
                       gu, g.W, g.N, g.tiles_per_face, nchunk, g.bound);
    return check_launch("query_ngp: point geometry");
}

// SirenNet in query mode (sdfr_query_siren_forward): field_p_kernel at the caller's points,
// as NgpQueryNet is field_r_kernel's.  The SIREN has no gather stage, so there is no
// staging kernel either: a lane reads its point (12 bytes of points [B,R,N,3], passed in
// XFieldArgs::enc) where the render forms its sample from the ray -- 12 bytes per 1.1
// MFLOP of MLP.  Same packed weights (sdfr_render_siren_pack), FiLM vectors and k-step
// order as the render.
struct SirenQueryNet : SirenNet {
    static constexpr bool kQuery = true;
};
static_assert(PNet<SirenQueryNet>::kSteps == PNet<SirenNet>::kSteps &&
                  SirenQueryNet::kSlices == SirenNet::kSlices && kPTiles * kTileRays == 32 &&
                  kPSamples == 4,
              "the query runs the render's k-steps on the render's packing");

// The field kernel in query mode.  g: B faces, H = 1, W = R, N points per group, cam = dirs
// [B,R,3]; in: the gathered enc (ngp) or the points [B,R,N,3] (SIREN); xws: the packed
// weights' region (workspace or the caller's prepacked buffer).
int launch_qfield(int net, const NetPtrs &P, const GeomArgs &g, const float *in, const char *xws,
                  const float *film, float *sdf, float *rgb, hipStream_t st) {
    XFieldArgs f{};
    f.g = g;
    f.enc = in;
    f.sdf = sdf;
    f.rgb = rgb;
    f.nseg = 1;
    if (net == kNetNgp) {
        fill_xfield_weights<NgpQueryNet>(f, P, xws, film);
        const uint32_t blocks = g.B * ((g.tiles_per_face + kRTiles - 1) / kRTiles);
        hipLaunchKernelGGL((field_r_kernel<NgpQueryNet>), dim3(blocks), dim3(kRThreads), 0, st, f);
        return check_launch("query_ngp: field (f16x3)");
    }
    fill_xfield_weights<SirenQueryNet>(f, P, xws, film);
    const uint32_t blocks = g.B * ((g.tiles_per_face + kPTiles - 1) / kPTiles);
    hipLaunchKernelGGL((field_p_kernel<SirenQueryNet>), dim3(blocks), dim3(kPThreads), 0, st, f);
    return check_launch("query_siren: field (f16x3)");
}

}  // namespace sdfr

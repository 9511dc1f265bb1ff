// field_fc_query.hip -- the fused FC field (FCGenerator) evaluated at caller-supplied points
// (sdfr_query_fc_forward; entry point in render_api.hip):
//
//   field_r_kernel<FcQueryNet>   the FC render's split-fp16 MLP with the point and the
//                                group's direction read from memory, no compositing, and a
//                                per-sample store of the SDF and the colour
//
// The FC network has no gather stage, so there is no staging kernel: a lane reads its point
// (12 bytes of points [B,R,N,3], passed in XFieldArgs::enc) where the render forms its
// sample from the ray, halves it as the render does (pin = RN(p / 2)) and builds the 60
// positional encodings from it with the render's posenc_val.  Same packed weights
// (sdfr_render_fc_pack), FiLM slots (1/su and the bias, layer 0's per face with
// style_in(styles)) and k-step order as the render: a point the render samples gets the
// render's SDF bit for bit.
//
// A unit of its own: field_query.hip already instantiates field_r_kernel (NgpQueryNet), and
// co-compiled instantiations of one kernel template share register-allocation context, so
// a second one there would move the ngp query kernel's code.  Built with the field units'
// flags.
#include "field_r.h"

namespace sdfr {

// FcNet in query mode, as NgpQueryNet is NgpNet's.
struct FcQueryNet : FcNet {
    static constexpr bool kQuery = true;
};
static_assert(RNet<FcQueryNet>::kSteps == RNet<FcNet>::kSteps &&
                  FcQueryNet::kSlices == FcNet::kSlices,
              "the query runs the render's k-steps on the render's packing");

// g: B faces, H = 1, W = R, N points per group, cam = dirs [B,R,3]; points [B,R,N,3]; xws:
// the packed weights' region (workspace or the caller's prepacked buffer).
int launch_qfield_fc(const NetPtrs &P, const GeomArgs &g, const float *points, const char *xws,
                     const float *film, float *sdf, float *rgb, hipStream_t st) {
    XFieldArgs f{};
    f.g = g;
    f.enc = points;
    f.sdf = sdf;
    f.rgb = rgb;
    f.nseg = 1;
    fill_xfield_weights<FcQueryNet>(f, P, xws, film);
    const uint32_t blocks = g.B * ((g.tiles_per_face + kRTiles - 1) / kRTiles);
    hipLaunchKernelGGL((field_r_kernel<FcQueryNet>), dim3(blocks), dim3(kRThreads), 0, st, f);
    return check_launch("query_fc: field (f16x3)");
}

}  // namespace sdfr

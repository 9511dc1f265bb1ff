// render_launch.h -- the launch functions that the renderer's kernel units export to the
// entry points (render_api.hip).  Host declarations only: every function enqueues its
// kernels on `st` and returns SDFR_OK or the failed launch's code (check_launch).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "render_ngp.h"

namespace sdfr {

// The networks of the split-fp16 field path, numbered as sdfr_render_pack_bytes(net).
enum : int { kNetNgp = 0, kNetSiren = 1, kNetFc = 2 };
constexpr int kMaxLayers = 9;
// FiLM sets per face in a call's `film` region ([B][films][2][256]; ngp: kFilm)
constexpr uint32_t kSirenFilm = 9, kFcFilm = 9, kSirenGradFilm = 8;

// A network's tensors in policy order (layer 0, dense layers, views; FiLM sets); for ngp
// also the two reference layers that make the composed layer 0.
struct NetPtrs {
    const float *w[kMaxLayers], *b[kMaxLayers];
    const float *in_w, *in_b, *p0_w, *p0_b;
    const float *gw[kMaxLayers], *gb[kMaxLayers], *bw[kMaxLayers], *bb[kMaxLayers];
    const float *sigma_w, *sigma_b, *rgb_w, *rgb_b, *sigmoid_beta;
};

// ---- render_ngp.hip: the ngp render's own stages -----------------------------------
// fp32 path: FiLM vectors and the fp32 MFMA fragments
int launch_prep(const sdfr_ngp_weights *w, const sdfr_ngp_render_args *a, f4 *packed, float *film,
                hipStream_t st);
// the per-sample geometry (gu always, zd when non-null) and the hash-grid gather
int launch_geom(const GeomArgs &g, float2 *zd, f4 *gu, hipStream_t st);
int launch_encode(const sdfr_ngp_weights *w, const GeomArgs &g, float *enc, const f4 *gu,
                  hipStream_t st);
int launch_field_fp32(const sdfr_ngp_weights *w, const sdfr_ngp_render_args *a, const GeomArgs &g,
                      const float *enc, const f4 *packed, const float *film, hipStream_t st);
size_t fp32_packed_bytes();

// ---- field_f16x3.hip: the split-fp16 field path ------------------------------------
// Its weight region (`xws`, f16x3_ws_bytes(net)) holds the packed fp16 fragments, row
// scales and scaled biases: inside the call's workspace, or the caller's prepacked buffer.
size_t f16x3_ws_bytes(int net);
// FiLM vectors of the B faces' styles into `film` (null: none), and with `pack` the row
// scales and the weight packing into xws
int launch_xprep(int net, const NetPtrs &P, uint32_t B, const float *styles, char *xws,
                 float *film, bool pack, hipStream_t st);
int launch_xfield(int net, const NetPtrs &P, const sdfr_ngp_render_args *a, const GeomArgs &g,
                  const float *enc, const char *xws, const float *film, hipStream_t st,
                  float *part, const float2 *zd);
// the per-row power-of-two scales of `layers` weight matrices [256][K[l]]
int launch_xscale(const float *const *w, const float *const *b, const uint32_t *K, int layers,
                  float *su, float *bias_s, hipStream_t st);
// sample-segment split of the field kernel for small batches
constexpr uint32_t kFieldSplitMax = 4;   // sample segments per ray at most
uint32_t field_nseg(uint32_t B, uint32_t tiles_per_face, uint32_t N, int force_background,
                    uint32_t max_seg);
size_t field_part_bytes(uint32_t B, uint32_t tiles_per_face, uint32_t N);

// ---- field_query.hip: the field at caller points -----------------------------------
// g in query mode: H = 1, W = R groups, N points per group, cam = dirs [B,R,3];
// sdf [B,R,N], rgb [B,R,N,3] or null.  ngp: the points' grid coordinates gu in tile order,
// then field_r_kernel on `in` = the gathered enc; SIREN: field_p_kernel on `in` = the
// points [B,R,N,3].
int launch_query_geom(const float *points, f4 *gu, const GeomArgs &g, hipStream_t st);
int launch_qfield(int net, const NetPtrs &P, const GeomArgs &g, const float *in, const char *xws,
                  const float *film, float *sdf, float *rgb, hipStream_t st);

// ---- field_fc_query.hip: the FC field at caller points ------------------------------
// g as for launch_qfield; field_r_kernel on the points [B,R,N,3] themselves
int launch_qfield_fc(const NetPtrs &P, const GeomArgs &g, const float *points, const char *xws,
                     const float *film, float *sdf, float *rgb, hipStream_t st);

// ---- field_grad.hip: SDF and gradient at caller points ------------------------------
constexpr uint32_t kGradPts = 8;             // points per wave pass: the padding unit of M
constexpr uint32_t kGradPointBytes = 4 * kFeatIn * sizeof(float);   // gd per padded point
// ngp: the gather with input derivatives, gd [B Mp][4][32], Mp = M rounded up to kGradPts
int launch_grad_gather(const sdfr_ngp_weights *w, const float *points, float *gd, uint32_t B,
                       uint32_t M, uint32_t Mp, hipStream_t st);
// the forward-mode field kernel (net: kNetNgp on the gather's gd with the grid's `bound`,
// kNetSiren and kNetFc on the points [B,M,3] themselves; kNetFc on the render's xws and
// film of launch_xprep); sdf [B,M] or null, grad [B,M,3]
int launch_gfield(int net, const NetPtrs &P, const char *xws, const float *film, const float *in,
                  float *sdf, float *grad, uint32_t B, uint32_t M, float bound, hipStream_t st);
// SIREN: the SDF trunk in field_r_kernel's packing (siren_grad_pack_bytes(): packed slices |
// su [8][256] | bias_s [8][256]); FiLM vectors film [B][8][2][256] and, with `pack`, the row
// scales and the packing into xws (B = 0, film null: packing only)
size_t siren_grad_pack_bytes();
int launch_gprep_siren(const NetPtrs &P, uint32_t B, const float *styles, char *xws, float *film,
                       bool pack, hipStream_t st);

// ---- geometry.hip: the geometry render's own kernels --------------------------------
// The cameras' samples in plain [B,H,W,N] order as the gradient gather's points (pnet
// [S,3], zd [S] = (z, dist), S = B H W N), and the compositing of the gradient call's
// sdf [S] / gnet [S,3] into per-sample eikonal [S,3] and the normal / depth / xyz / mask
// maps (each output may be null).
int launch_geom_points(const GeomArgs &g, float *pnet, float2 *zd, hipStream_t st);
int launch_geom_composite(const GeomArgs &g, const float2 *zd, const float *sdf,
                          const float *gnet, const float *sigmoid_beta, int force_background,
                          float *eikonal, float *normal, float *depth, float *xyz, float *mask,
                          hipStream_t st);

// ---- surface.hip: the surface render's ray-side kernels -----------------------------
// rays = B H W.  bracket: the coarse sdf [rays][N] and zd [rays N] (geom_points_kernel's) ->
// br [rays] = (a, b, fa, fb) and sidx [rays] = s* or -1.  step: the bracket narrowed by f
// [B][Mp] (the SDF at the previous midpoints; null on the first step), then the next
// midpoints' network coordinates pts [B][Mp][3]; Mp = H W rounded up to 32, the padding
// points get the origin.  hit: the last narrowing (f null: none), then zs [rays] = z*, the
// hit points' network coordinates pnet [rays][3] and the rays' view directions dirs
// [rays][3].  maps: the [B,C,H,W] outputs (each may be null) from sidx, zs, the gradient
// call's gsdf [rays] / ggrad [rays][3] and the colour query's rgbq [rays][3] (each read only
// for the outputs that need it).
int launch_surf_bracket(const GeomArgs &g, const float *sdf, const float2 *zd, f4 *br,
                        int32_t *sidx, hipStream_t st);
int launch_surf_step(const GeomArgs &g, uint32_t Mp, const float *f, f4 *br, float *pts,
                     hipStream_t st);
int launch_surf_hit(const GeomArgs &g, uint32_t Mp, const float *f, const f4 *br,
                    const int32_t *sidx, float *zs, float *pnet, float *dirs, hipStream_t st);
int launch_surf_maps(const GeomArgs &g, const int32_t *sidx, const float *zs, const float *gsdf,
                     const float *ggrad, const float *rgbq, float *hit, int32_t *sample,
                     float *depth, float *residual, float *xyz, float *normal, float *rgb,
                     hipStream_t st);

}  // namespace sdfr

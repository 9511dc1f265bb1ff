/*
 * sdfr.h -- C ABI of libsdfr.so, the MI355X (gfx950) SDF + hash-grid renderer.
 *
 * Plain pointers and sizes only; every pointer below is a DEVICE pointer
 * unless stated otherwise, `stream` is a hipStream_t passed as void*
 * (NULL = the legacy default stream).  All entry points are asynchronous
 * with respect to the host, enqueue on `stream`, return SDFR_OK (0) or a
 * negative status, and never allocate device memory.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   sdfr_grid_encode_forward   <- grid_encode_forward
 *        im2scene/sdf/models/gridencoder/src/gridencoder.h:11,
 *        pybind export gridencoder/src/bindings.cpp:5, caller grid.py:54
 *   sdfr_grid_encode_backward  <- grid_encode_backward
 *        gridencoder.h:12, bindings.cpp:6, caller grid.py:84
 *   sdfr_sh_encode_forward     <- sh_encode_forward
 *        shencoder/src/shencoder.h:9, bindings.cpp:5, caller sphere_harmonics.py:32
 *   sdfr_sh_encode_backward    <- sh_encode_backward
 *        shencoder.h:10, bindings.cpp:6, caller sphere_harmonics.py:51
 *   sdfr_render_ngp_forward    <- VolumeFeatureRenderer.forward for
 *        rendering.type == "ngp" (sdf_model.py:411-423 -> render :363 ->
 *        render_rays :310 -> NGPSIRENGenerator.forward :1566 ->
 *        volume_integration :236).  The reference has no native op here;
 *        this one fuses the whole chain.
 *
 * Error behaviour mirrors the reference: the same argument combinations the
 * reference rejects with std::runtime_error / TORCH_CHECK return
 * SDFR_EINVAL here, with the reference's message in sdfr_last_error().
 */
#ifndef SDFR_H_
#define SDFR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFR_OK 0
#define SDFR_EINVAL (-1)       /* bad sizes / unsupported D, C, degree        */
#define SDFR_ELAUNCH (-2)      /* HIP launch or runtime error                 */
#define SDFR_EUNSUPPORTED (-3) /* valid for the reference, not implemented    */

#define SDFR_ABI_VERSION 15

int sdfr_abi_version(void);
/* Thread-local message for the last non-zero status of this thread. */
const char *sdfr_last_error(void);

/* ---------------------------------------------------------------------------
 * Multiresolution hash / tiled grid encoder (gridencoder.cu semantics).
 *   inputs      [B, D] fp32 in [0,1] (outside -> output 0)
 *   embeddings  [offsets[L], C] fp32
 *   offsets     [L+1] int32
 *   outputs     [L, B, C] fp32 (level-major, as the reference)
 *   dy_dx       [B, L*D*C] fp32 or NULL
 *   S = log2(per_level_scale) (fp32), H = base resolution
 *   gridtype 0 = hash, 1 = tiled; interp 0 = linear, 1 = smoothstep
 *   D in {2,3,4,5}, C in {1,2,4,8}; L <= 64.
 * ------------------------------------------------------------------------- */
int sdfr_grid_encode_forward(const float *inputs, const float *embeddings,
                             const int32_t *offsets, float *outputs,
                             uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                             float S, uint32_t H, float *dy_dx,
                             uint32_t gridtype, int align_corners,
                             uint32_t interp, void *stream);

/*   grad            [L, B, C]
 *   grad_embeddings [offsets[L], C], must be zeroed by the caller (grid.py:75); may be
 *                   NULL when grad_inputs is given (input gradient only: the eikonal
 *                   term's pass, whose table gradient autograd.grad discards)
 *   dy_dx / grad_inputs: both NULL, or dy_dx [B, L*D*C] and grad_inputs [B, D]
 *   (grad_inputs is overwritten). */
int sdfr_grid_encode_backward(const float *grad, const float *inputs,
                              const float *embeddings, const int32_t *offsets,
                              float *grad_embeddings, uint32_t B, uint32_t D,
                              uint32_t C, uint32_t L, float S, uint32_t H,
                              const float *dy_dx, float *grad_inputs,
                              uint32_t gridtype, int align_corners,
                              uint32_t interp, void *stream);

/* The same with a caller-owned device workspace of at least
 * sdfr_grid_encode_backward_ws_bytes(...) bytes (0 = none needed: then ws may be
 * NULL).  With it, the table gradient of the fine levels is binned and summed in
 * LDS instead of scattered with global atomics (csrc/encoders.hip); with ws NULL
 * or too small, the workspace-free path runs (LDS windows for the coarse levels,
 * direct atomics for the hashed ones).  sdfr_grid_encode_backward is this function
 * with ws NULL: it allocates nothing (stream-ordered, HIP-graph-capture safe). */
size_t sdfr_grid_encode_backward_ws_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                          float S, uint32_t H, int align_corners);
int sdfr_grid_encode_backward_ws(const float *grad, const float *inputs,
                                 const float *embeddings, const int32_t *offsets,
                                 float *grad_embeddings, uint32_t B, uint32_t D,
                                 uint32_t C, uint32_t L, float S, uint32_t H,
                                 const float *dy_dx, float *grad_inputs,
                                 uint32_t gridtype, int align_corners,
                                 uint32_t interp, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Real spherical harmonics (shencoder.cu semantics), C = degree.
 *   inputs [B, D], D must be 3; outputs [B, C*C]; dy_dx [B, D*C*C] or NULL.
 *   Degrees 1..8 are implemented (SDFace uses 4; 5..8 from the bands that
 *   csrc/sh_gen.py generates); other degrees -> SDFR_EUNSUPPORTED.
 * ------------------------------------------------------------------------- */
int sdfr_sh_encode_forward(const float *inputs, float *outputs, uint32_t B,
                           uint32_t D, uint32_t C, float *dy_dx, void *stream);

/* grad [B, C*C]; grad_inputs [B, D] accumulated into (caller zeroes it). */
int sdfr_sh_encode_backward(const float *grad, const float *inputs, uint32_t B,
                            uint32_t D, uint32_t C, const float *dy_dx,
                            float *grad_inputs, void *stream);

/* ---------------------------------------------------------------------------
 * Fused NGP renderer forward (inference / frozen renderer).
 *
 * Network: NGPSIRENGenerator(D=2, W=256, style_dim=256) with a
 * GridEncoder(L=16, C=2, H=16, 2^19 rows, desired 4096) and SHEncoder(4).
 * Parameter pointers are the PyTorch tensors of the reference state dict
 * (row-major [out, in] weights, sdf_model.py:1545-1564).
 * ------------------------------------------------------------------------- */
typedef struct sdfr_ngp_weights {
    const float *embeddings;      /* [offsets[L], 2]                              */
    const int32_t *offsets;       /* [L+1] (device)                               */
    uint32_t num_levels;          /* L (16)                                        */
    float log2_per_level_scale;   /* S                                            */
    uint32_t base_resolution;     /* H (16)                                        */
    float bound;                  /* NGPSIRENGenerator.bound (2)                   */
    const float *input_w, *input_b;     /* [256,32], [256]                        */
    const float *pts_w[3], *pts_b[3];   /* [256,256], [256]                       */
    const float *pts_gw[3], *pts_gb[3]; /* gamma LinearLayer [256,256], [256]     */
    const float *pts_bw[3], *pts_bb[3]; /* beta  LinearLayer [256,256], [256]     */
    const float *views_w, *views_b;     /* [256,272], [256]                       */
    const float *views_gw, *views_gb, *views_bw, *views_bb;
    const float *sigma_w, *sigma_b;     /* [1,256], [1]                           */
    const float *rgb_w, *rgb_b;         /* [3,256], [3]                           */
    const float *sigmoid_beta;          /* [1] (renderer.sigmoid_beta)            */
} sdfr_ngp_weights;

typedef struct sdfr_ngp_render_args {
    uint32_t B, H, W, N;          /* faces, image rows, cols, samples per ray      */
    const float *cam;             /* [B,3,4] c2w = [R^T | T]                       */
    const float *focal;           /* [B]                                           */
    const float *near_;           /* [B]                                           */
    const float *far_;            /* [B]                                           */
    const float *styles;          /* [B,256] renderer latent                       */
    const float *pix_x;           /* [W] renderer i-buffer row (x + 0.5)           */
    const float *pix_y;           /* [H] renderer j-buffer column                  */
    const float *t_vals;          /* [N]                                           */
    const float *t_rand;          /* NULL, [B,H,W] or [B,H,W,N]                    */
    const float *sigma_noise;     /* NULL or [B,H,W,N] (no_sdf mode only)          */
    int t_rand_per_sample;        /* 1 -> t_rand is [B,H,W,N] (stratified)         */
    int offset_sampling;          /* !opt.no_offset_sampling                       */
    int static_viewdirs;
    int z_normalize;              /* !opt.no_z_normalize                           */
    int force_background;
    int with_sdf;                 /* !opt.no_sdf                                   */
    float *rgb;                   /* [B,3,H,W]                     (required)      */
    float *features;              /* [B,256,H,W] or NULL                            */
    float *sdf;                   /* [B,H,W,N] or NULL                             */
    float *xyz;                   /* [B,3,H,W] or NULL                             */
    float *mask;                  /* [B,1,H,W] or NULL                             */
    void *workspace;              /* >= sdfr_render_ngp_workspace_bytes()          */
    size_t workspace_bytes;
    /* Optional hipEvent_t handles (NULL = skip), recorded on `stream`:
     * [0] at entry, [1] before the hash-grid kernel, [2] after it (ngp f16x3;
     * before the FiLM prep), [3] after the field (MLP + compositing) kernel. */
    void *stage_events[4];
    /* Field-stage GEMM arithmetic (both accumulate in fp32):
     * SDFR_FIELD_F16X3 (0, default) three v_mfma_f32_16x16x32_f16 per tile on a
     *   hi/lo fp16 split of row-scaled weights and activations (fp32-level
     *   accuracy);
     * SDFR_FIELD_FP32 (1) v_mfma_f32_16x16x4_f32 (exact fp32 fma chain). */
    int field_precision;
    /* NULL, or the split-fp16 weights packed beforehand by sdfr_render_ngp_pack /
     * sdfr_render_siren_pack from the SAME weights (f16x3 only): the per-call
     * row-scale and packing kernels are then skipped, only the per-face FiLM
     * vectors are formed. */
    const void *prepacked;
    /* Upper bound on the sample segments per ray of the f16x3 field stage (0 = the
     * default 4): batches too small to give every CU a workgroup split each ray's
     * samples over up to this many workgroups and chain the segments in a merge
     * kernel (sdf_model.py:273-289's cumprod re-associated: fp32-rounding-level
     * differences).  1 disables the split; 2 or 4 otherwise.  The workspace size
     * (sdfr_render_ngp_workspace_bytes) covers the default bound. */
    uint32_t max_field_segments;
    /* ABI 11.  styles_event: NULL, or a hipEvent_t that `stream` waits on before the
     * first use of `styles` (the FiLM prep; the ngp f16x3 path enqueues the sample
     * geometry and the hash-grid gather ahead of that wait, so a caller may still be
     * computing the styles on another stream).  field_event: NULL, or a hipEvent_t
     * recorded right before the field kernel (after the FiLM prep). */
    void *styles_event;
    void *field_event;
    /* ABI 12 (f16x3 ngp / FC only): NULL, or [B,H,W,32,2,8] fp16 -- the features
     * times features_mod[b,c] in the decoder's split-NHWC layout (hi / lo halves of
     * each 8-channel group, sdfr_modulate_to_nhwc_split's output, bit for bit), written
     * instead of the NCHW `features` (which must then be NULL). */
    void *features_split;
    const float *features_mod;    /* [B,256] with features_split                    */
} sdfr_ngp_render_args;

#define SDFR_FIELD_F16X3 0
#define SDFR_FIELD_FP32 1

size_t sdfr_render_ngp_workspace_bytes(uint32_t B, uint32_t H, uint32_t W,
                                       uint32_t N, uint32_t num_levels);

int sdfr_render_ngp_forward(const sdfr_ngp_weights *w,
                            const sdfr_ngp_render_args *a, void *stream);

/* ---------------------------------------------------------------------------
 * Fused SIREN renderer forward (rendering.type == "sdf", SirenGenerator,
 * sdf_model.py:101-139, BASELINE configs[4]): the same render chain as
 * sdfr_render_ngp_forward with the network's 8 FiLM layers fed by the
 * normalised sample points and the views layer by the unit view direction.
 * Replaces VolumeFeatureRenderer.forward for type "sdf" (sdf_model.py:411-423);
 * the reference has no native op here.  Takes the same render args
 * (field_precision must be SDFR_FIELD_F16X3); workspace from
 * sdfr_render_siren_workspace_bytes(B).  stage_events[1] == [2] (no encode stage).
 * ------------------------------------------------------------------------- */
typedef struct sdfr_siren_weights {
    uint32_t depth;                     /* D (8)                                    */
    uint32_t width;                     /* W (256)                                  */
    const float *pts_w[8], *pts_b[8];   /* [256,3] (layer 0) / [256,256], [256]     */
    const float *pts_gw[8], *pts_gb[8]; /* gamma LinearLayer [256,256], [256]       */
    const float *pts_bw[8], *pts_bb[8]; /* beta  LinearLayer [256,256], [256]       */
    const float *views_w, *views_b;     /* [256,259], [256]                         */
    const float *views_gw, *views_gb, *views_bw, *views_bb;
    const float *sigma_w, *sigma_b;     /* [1,256], [1]                             */
    const float *rgb_w, *rgb_b;         /* [3,256], [3]                             */
    const float *sigmoid_beta;          /* [1] (renderer.sigmoid_beta)              */
} sdfr_siren_weights;

size_t sdfr_render_siren_workspace_bytes(uint32_t B);

/* ---------------------------------------------------------------------------
 * Fused FCGenerator renderer forward (rendering.fc == 1, sdf_model.py:1599-1670:
 * the "plain Fourier MLP" of BASELINE configs[4]): positional encodings of the
 * normalised sample point (10 frequencies) -> x_in + style_in(styles) -> ReLU ->
 * 7 x (Linear 256, ReLU) -> sigma | [h, encodings of the view direction (4
 * frequencies)] -> views_linears (the colour features) -> rgb_linear, then the
 * same SDF -> density and compositing as the other networks
 * (sdf_model.py:231-301).  Replaces VolumeFeatureRenderer.forward for fc == 1
 * (sdf_model.py:411-423).  Same render args (field_precision must be
 * SDFR_FIELD_F16X3); workspace from sdfr_render_fc_workspace_bytes.
 * stage_events[1] == [2] (no encode stage).
 * ------------------------------------------------------------------------- */
typedef struct sdfr_fc_weights {
    uint32_t depth;                     /* D (8)                                    */
    uint32_t width;                     /* W (256)                                  */
    const float *x_in_w, *x_in_b;       /* [256,60], [256]                          */
    const float *style_w, *style_b;     /* style_in [256,256], [256]                */
    const float *pts_w[7], *pts_b[7];   /* [256,256], [256]                         */
    const float *views_w, *views_b;     /* [256,280], [256]                         */
    const float *sigma_w, *sigma_b;     /* [1,256], [1]                             */
    const float *rgb_w, *rgb_b;         /* [3,256], [3]                             */
    const float *sigmoid_beta;          /* [1] (renderer.sigmoid_beta)              */
} sdfr_fc_weights;

size_t sdfr_render_fc_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N);

int sdfr_render_fc_forward(const sdfr_fc_weights *w,
                           const sdfr_ngp_render_args *a, void *stream);

/* Split-fp16 weight packing of the field kernel (row scales, scaled biases, MFMA
 * A-fragments), done once per weight version by the caller instead of per call:
 * `packed` holds sdfr_render_pack_bytes(net) bytes (net 0 ngp, 1 siren, 2 fc). */
size_t sdfr_render_pack_bytes(int net);
int sdfr_render_ngp_pack(const sdfr_ngp_weights *w, void *packed, void *stream);
int sdfr_render_siren_pack(const sdfr_siren_weights *w, void *packed, void *stream);
int sdfr_render_fc_pack(const sdfr_fc_weights *w, void *packed, void *stream);

int sdfr_render_siren_forward(const sdfr_siren_weights *w,
                              const sdfr_ngp_render_args *a, void *stream);

/* Profiling aid: enqueue only the hash-grid stage of the fused renderer
 * (writes the encoded samples into the workspace).  Same arguments. */
int sdfr_render_ngp_encode_only(const sdfr_ngp_weights *w,
                                const sdfr_ngp_render_args *a, void *stream);

/* ---------------------------------------------------------------------------
 * Fused NGP field query at caller-supplied points (ABI 14; no reference native op:
 * replaces NGPSIRENGenerator.forward, sdf_model.py:1566-1592, evaluated op by op on
 * cat([points, dirs]) -- e.g. on a cube of points for marching cubes, or at mesh
 * vertices for their colour).  The hash-grid gather and the split-fp16 field kernel of
 * sdfr_render_ngp_forward with the caller's points in place of the ray sampler and a
 * per-sample store in place of compositing: the same packed weights, FiLM vectors and
 * per-sample arithmetic (f16x3 only), so a point the render samples gets the render's
 * SDF bit for bit.  A point whose grid coordinate leaves [0,1] in any axis gets zero
 * grid features and still runs through the MLP (GridEncoder, gridencoder.cu:104-111).
 * Points are grouped: the N points of a group share one view direction.  The kernel
 * takes two points of a group per pass, so N = 1 (a direction per point) idles half
 * of its lanes.  The colour head runs whether or not rgb is wanted.
 * SDFR_EINVAL before any launch for null pointers, zero sizes, a workspace below
 * sdfr_query_ngp_workspace_bytes(B, R, N) (about 144 bytes per point of the padded
 * count B ceil(R/16) 16 N) or 2^25 or more padded points in one call.
 * ------------------------------------------------------------------------- */
/* One argument struct for the three networks' query calls; sdfr_{ngp,siren,fc}_query_args
 * name it per network (the SIREN and FC calls' comments below say what differs). */
typedef struct sdfr_query_args {
    uint32_t B, R, N;        /* faces; direction groups per face; points per group      */
    const float *points;     /* [B,R,N,3] NETWORK coordinates: what the network's        */
                             /* .forward receives (normalized_pts, sdf_model.py:349);    */
                             /* ngp: the grid coordinate u = (p + bound) / (2 bound) is   */
                             /* formed inside with the rounded ops of grid.py:149         */
    const float *dirs;       /* [B,R,3] view direction of each group AS THE NETWORK SEES  */
                             /* IT (already unit length; not normalised again)            */
    const float *styles;     /* [B,256] renderer latent                                   */
    float *sdf;              /* [B,R,N]   sigma_linear output           (required)        */
    float *rgb;              /* [B,R,N,3] sigmoid(rgb_linear) in [0,1], or NULL           */
    void *workspace; size_t workspace_bytes;
    const void *prepacked;   /* as sdfr_ngp_render_args.prepacked (the network's own      */
                             /* sdfr_render_*_pack buffer), or NULL                       */
} sdfr_query_args;
typedef sdfr_query_args sdfr_ngp_query_args;
size_t sdfr_query_ngp_workspace_bytes(uint32_t B, uint32_t R, uint32_t N);
int sdfr_query_ngp_forward(const sdfr_ngp_weights *w, const sdfr_ngp_query_args *a, void *stream);

/* ---------------------------------------------------------------------------
 * Fused SDF and its exact gradient at caller-supplied points (ABI 15; replaces autograd
 * through NGPSIRENGenerator's SDF trunk, as get_eikonal_term uses it, sdf_model.py:224-229).
 * A gather that stores, per point, the 32 hash-grid features and their derivatives with
 * respect to the grid coordinate (the values and dy_dx of sdfr_grid_encode_forward, bit
 * for bit), then a forward-mode split-fp16 field kernel over the SDF trunk (composed
 * layer 0, pts_linears.1-2, sigma_linear; no views layer, no colour): the value and its
 * three tangents are four MFMA columns of the query's GEMM stream on the same packed
 * weights (their first 34 slices) and FiLM vectors.  sdf is the query's SDF bit for bit;
 * grad is d sdf / d point in NETWORK coordinates (the coordinates of `points`).  A point
 * whose grid coordinate leaves [0,1] in any axis has zero features and a zero gradient.
 * The hash grid is piecewise trilinear: on a cell face the gradient is that of the cell
 * the gather's floor() selects.
 * Workspace: 512 bytes per padded point (M rounded up to 8 per face; the region starts
 * with the gather's output [B][Mp][4 = value, d/du_0..2][32] fp32) + 8 KiB of FiLM vectors
 * per face + the weight-packing region.  SDFR_EINVAL before any launch for null
 * arguments or required pointers, zero sizes, a workspace below
 * sdfr_query_ngp_grad_workspace_bytes(B, M), or 2^25 or more padded points in one call
 * (the kernels index the gather's output in fp32 elements, 128 per padded point, with
 * 32-bit arithmetic; sdfr_query_ngp_grad_workspace_bytes returns 0 for such a size);
 * SDFR_EUNSUPPORTED for num_levels != 16.
 * ------------------------------------------------------------------------- */
/* One argument struct for the three networks' gradient calls, named per network. */
typedef struct sdfr_grad_args {
    uint32_t B, M;            /* faces; points per face                        */
    const float *points;      /* [B,M,3] network coordinates                   */
    const float *styles;      /* [B,256]                                       */
    float *sdf;               /* [B,M] or NULL                                 */
    float *grad;              /* [B,M,3] d sdf / d point (network coordinates) */
    void *workspace; size_t workspace_bytes;
    const void *prepacked;    /* as sdfr_query_args.prepacked, or NULL (SIREN: */
                              /* sdfr_query_siren_grad_pack's buffer)          */
} sdfr_grad_args;
typedef sdfr_grad_args sdfr_ngp_grad_args;
size_t sdfr_query_ngp_grad_workspace_bytes(uint32_t B, uint32_t M);
int sdfr_query_ngp_grad(const sdfr_ngp_weights *w, const sdfr_ngp_grad_args *a, void *stream);

/* ---------------------------------------------------------------------------
 * Geometry render: the SDF gradient along the camera rays of a render, and normal, depth
 * and xyz maps composited with the render's weights (added to ABI 15 without a version
 * step: the two entry points below are additive, nothing existing changes).  Replaces
 * VolumeFeatureRenderer.forward(return_eikonal=True)'s autograd pass (get_eikonal_term,
 * sdf_model.py:224-229) at inference.
 * The samples are those of sdfr_render_ngp_forward for the same cameras, t_vals, t_rand
 * and sampling flags, in plain [B,H,W,N] order.  They run through sdfr_query_ngp_grad's
 * gather and forward-mode field kernel as B x (H W N) points, then one compositing kernel:
 *   sdf      [B,H,W,N]    the render's return_sdf output, bit for bit
 *   eikonal  [B,H,W,N,3]  d sdf / d world point: the network-coordinate gradient g times
 *                         2 / (far - near) when z_normalize (fdiv(fmul(g, 2), far - near)),
 *                         g otherwise; zero for a sample outside the grid's box
 *   normal   [B,3,H,W]    sum_s w_s eikonal_s (not normalised)
 *   depth    [B,1,H,W]    sum_s w_s z_s
 *   xyz      [B,3,H,W]    sum_s w_s (o + d z_s), world points, as the render's xyz
 *   mask     [B,1,H,W]    w_{N-1}
 * with the render's weights, front to back in fp32: sigma = sigmoid(-sdf / beta) / beta,
 * alpha = 1 - exp(-sigma dist), w = alpha T (the last sample's w = 1 - sum of the others
 * under force_background), T <- T ((1 - alpha) + 1e-10).  Every output may be NULL, at
 * least one is required.  pix_y may be the renderer's buffer offset by y0 with H = a band
 * of rows (W stays the image width: the ray directions use W / 2 for both axes).
 * Workspace: sdfr_query_ngp_grad's for (B, M = H W N) (512 bytes per padded point, M
 * rounded up to 8 per face, + 8 KiB of FiLM vectors per face + the weight-packing region),
 * then 36 bytes per padded point: the network coordinates [P][3], (z, dist) [P][2], the
 * SDF [P] (unused when `sdf` is given) and the network-coordinate gradient [P][3], each
 * region rounded up to 256 bytes.  SDFR_EINVAL before any launch for null arguments or
 * required pointers, zero sizes, every output null, a null sigmoid_beta in the weights
 * (no SDF: no gradient), a workspace below sdfr_render_ngp_geometry_workspace_bytes, or
 * B x (H W N rounded up to 8) >= 2^25 (the gradient kernels' 32-bit indexing; the size
 * function returns 0 for such a size); SDFR_EUNSUPPORTED for num_levels != 16.
 * ------------------------------------------------------------------------- */
typedef struct sdfr_ngp_geometry_args {
    uint32_t B, H, W, N;          /* faces, image rows, cols, samples per ray      */
    const float *cam, *focal, *near_, *far_, *styles, *pix_x, *pix_y, *t_vals;
    const float *t_rand;          /* as sdfr_ngp_render_args; t_rand may be NULL   */
    int t_rand_per_sample, offset_sampling, z_normalize, force_background;
    float *sdf, *eikonal, *normal, *depth, *xyz, *mask;
    void *workspace; size_t workspace_bytes;
    const void *prepacked;        /* as sdfr_ngp_query_args.prepacked, or NULL     */
} sdfr_ngp_geometry_args;
size_t sdfr_render_ngp_geometry_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N);
int sdfr_render_ngp_geometry(const sdfr_ngp_weights *w, const sdfr_ngp_geometry_args *a,
                             void *stream);

/* ---------------------------------------------------------------------------
 * Fused SIREN field query at caller-supplied points (added to ABI 15 without a version
 * step: additive, nothing existing changes; no reference native op: replaces
 * SirenGenerator.forward, sdf_model.py:101-139, evaluated op by op on cat([points, dirs])).
 * The field kernel of sdfr_render_siren_forward with the caller's points in place of the
 * ray sampler and a per-sample store in place of compositing: the same packed weights
 * (`prepacked` is sdfr_render_siren_pack's buffer), FiLM vectors, k-step order and
 * per-sample arithmetic, so a point the render samples gets the render's SDF bit for bit.
 * The fields mean what sdfr_ngp_query_args' mean: points are NETWORK coordinates, the N
 * points of a group share one direction, directions are as the network sees them and are
 * not renormalised.  The SIREN has no grid box: every point runs through the same
 * arithmetic.
 * Rate: a wave pair of the kernel takes kPSamples = 4 points of each of 8 groups per
 * pass, so N = 1 (a direction per point) idles three quarters of its columns, N = 2 half,
 * N = 3 a quarter; N a multiple of 4 runs at the full rate.  The colour head runs whether
 * or not rgb is wanted.
 * Coordinate range: the kernel splits each coordinate into fp16 hi + lo parts without a
 * scale (the render's arithmetic, kept for the bit-identity above), which is finite below
 * 65504 and carries a relative error of 2^-22 per coordinate; the accuracy bounds of the
 * test-suite (against a float64 evaluation, relative to the fp32 module) are checked for
 * |coordinate| <= 64, the supported range.  The render's samples stay below 1.3.
 * Workspace: 18 KiB of FiLM vectors per face + the weight-packing region
 * (sdfr_render_pack_bytes(1)); it does not grow with the point count.
 * SDFR_EINVAL before any launch for null arguments or required pointers, a null FiLM or
 * weight pointer, zero sizes, a workspace below sdfr_query_siren_workspace_bytes(B, R, N),
 * or 2^30 or more padded points B x (R rounded up to 16) x N in one call (the kernel
 * forms three times a point index in 32 bits; the size function returns 0 for such a
 * size, and for products that wrap); SDFR_EUNSUPPORTED for depth != 8 or width != 256.
 * Asynchronous on `stream`; allocates nothing.
 * ------------------------------------------------------------------------- */
typedef sdfr_query_args sdfr_siren_query_args; /* prepacked: sdfr_render_siren_pack's */
size_t sdfr_query_siren_workspace_bytes(uint32_t B, uint32_t R, uint32_t N);
int sdfr_query_siren_forward(const sdfr_siren_weights *w, const sdfr_siren_query_args *a,
                             void *stream);

/* ---------------------------------------------------------------------------
 * Fused SIREN SDF and its exact gradient at caller-supplied points (added to ABI 15
 * without a version step; replaces autograd through SirenGenerator's SDF trunk, as
 * get_eikonal_term uses it, sdf_model.py:224-229).  The forward-mode split-fp16 field
 * kernel of sdfr_query_ngp_grad over pts_linears.0-7 and sigma_linear (no views layer, no
 * colour): a wave's 32 MFMA columns are 8 points x {value, d/dx, d/dy, d/dz}; layer 0's
 * value column is the point, its tangent columns the unit vectors; every tangent column
 * is rescaled by a power of two per layer (FiLM gamma is about 30, so tangents grow by
 * orders of magnitude per layer) and the exponent is undone exactly at the end.
 * grad is d sdf / d point in NETWORK coordinates.  There is no grid box and so no
 * "outside => zero" rule.
 * The kernel runs on field_r_kernel's k-step loop (32x32x16 MFMA, one slice per k-step),
 * whose weight layout differs from the render's SIREN packing: the trunk is packed on its
 * own.  `prepacked` of THIS call is the buffer of sdfr_query_siren_grad_pack
 * (sdfr_query_siren_grad_pack_bytes() bytes), NOT sdfr_render_siren_pack's; NULL packs
 * into the workspace on every call.
 * sdf (optional) is the same SDF as sdfr_query_siren_forward's up to fp32 rounding: the
 * two kernels accumulate the same products in a different order, and this one scales
 * layer 0's inputs by a power of two before the fp16 split.  The test-suite bounds the
 * difference (tests/test_gpu_siren_query.py, profiles/siren_gradient_parity.json).
 * Coordinate range: any finite fp32 coordinate (layer 0's inputs are pre-scaled); the
 * accuracy bounds are checked for |coordinate| <= 64.
 * Workspace: 16 KiB of FiLM vectors per face + the trunk's packing region; it does not
 * grow with the point count.  SDFR_EINVAL before any launch for null arguments or
 * required pointers, a null FiLM or weight pointer (sigma_linear and pts_linears; the
 * colour layers are not read), zero sizes, a workspace below
 * sdfr_query_siren_grad_workspace_bytes(B, M), or 2^30 or more padded points
 * B x (M rounded up to 8) in one call (the size function returns 0 for such a size);
 * SDFR_EUNSUPPORTED for depth != 8 or width != 256.  Asynchronous; allocates nothing.
 * ------------------------------------------------------------------------- */
typedef sdfr_grad_args sdfr_siren_grad_args; /* prepacked: sdfr_query_siren_grad_pack's */
size_t sdfr_query_siren_grad_workspace_bytes(uint32_t B, uint32_t M);
size_t sdfr_query_siren_grad_pack_bytes(void);
int sdfr_query_siren_grad_pack(const sdfr_siren_weights *w, void *packed, void *stream);
int sdfr_query_siren_grad(const sdfr_siren_weights *w, const sdfr_siren_grad_args *a,
                          void *stream);

/* ---------------------------------------------------------------------------
 * Fused FC field query at caller-supplied points (added to ABI 15 without a version step:
 * additive, nothing existing changes; no reference native op: replaces
 * FCGenerator.forward, sdf_model.py:1599-1670, evaluated op by op on cat([points, dirs])).
 * The field kernel of sdfr_render_fc_forward with the caller's points in place of the ray
 * sampler and a per-sample store in place of compositing: the same packed weights
 * (`prepacked` is sdfr_render_fc_pack's buffer; NULL packs into the workspace), FiLM slots
 * (1/su and the bias, layer 0's bias per face including style_in(styles)), k-step order
 * and per-sample arithmetic.  The point is halved exactly as the render halves its sample
 * (RN(p / 2)) before the 60 positional encodings, so a point the render samples gets the
 * render's SDF bit for bit.
 * The fields mean what sdfr_siren_query_args' mean: points are NETWORK coordinates, the N
 * points of a group share one direction, directions are as the network sees them and are
 * not renormalised.  There is no grid box: every point runs through the same arithmetic.
 * Rate: a wave of the kernel takes kRSamples = 2 points of each of 16 groups per pass, so
 * N = 1 (a direction per point) idles half of its columns; even N runs at the full rate.
 * The colour head runs whether or not rgb is wanted.
 * Coordinate range: the encodings' arguments are the fp32 module's own (2^i pi p / 2,
 * reduced in fp64), so any finite coordinate is evaluated as the module evaluates it; the
 * accuracy bounds of the test-suite are checked for |coordinate| <= 2.2.
 * Workspace: 18 KiB of FiLM slots per face + the weight-packing region
 * (sdfr_render_pack_bytes(2)); it does not grow with the point count.
 * SDFR_EINVAL before any launch for null arguments or required pointers, a null weight
 * pointer, zero sizes, a workspace below sdfr_query_fc_workspace_bytes(B, R, N), or 2^30
 * or more padded points B x (R rounded up to 16) x N in one call (the kernel forms
 * group, tile and padded-sample indices in 32 bits; the limit is the SIREN call's, which
 * keeps all of them in range; the size function returns 0 for such a size, and for
 * products that wrap); SDFR_EUNSUPPORTED for depth != 8 or width != 256.
 * Asynchronous on `stream`; allocates nothing.
 * ------------------------------------------------------------------------- */
typedef sdfr_query_args sdfr_fc_query_args;  /* prepacked: sdfr_render_fc_pack's buffer */
size_t sdfr_query_fc_workspace_bytes(uint32_t B, uint32_t R, uint32_t N);
int sdfr_query_fc_forward(const sdfr_fc_weights *w, const sdfr_fc_query_args *a, void *stream);

/* ---------------------------------------------------------------------------
 * Fused FC SDF and its exact gradient at caller-supplied points (added to ABI 15 without a
 * version step; replaces autograd through FCGenerator's SDF trunk).  The forward-mode
 * split-fp16 field kernel of sdfr_query_ngp_grad over x_in, pts_linears.0-6 and
 * sigma_linear (no views layer, no colour): a wave's 32 MFMA columns are 8 points x
 * {value, d/dx, d/dy, d/dz}.  Layer 0's value column holds the 60 encodings as the render
 * forms them; tangent column k holds their derivatives with respect to coordinate k,
 * + cos(arg) c_i / 2 for a sine entry and - sin(arg) c_i / 2 for a cosine entry, with the
 * module's own fp32 argument arg = RN(c_i RN(p_k / 2)), c_i = RN32(2^i pi).  Every layer is
 * ReLU: a tangent passes (1/su) z where the value's pre-activation is > 0 and is 0
 * elsewhere -- at exactly 0 the derivative is 0, as torch.relu's backward has it.  The
 * gradient is that of the piecewise linear trunk on the point's own piece; it jumps
 * where a pre-activation changes sign.  Tangent columns are rescaled by a power of two per
 * layer and the exponent is undone exactly at the end, so gradients of any magnitude
 * (1e-8 with nearly dead late layers, 1e+3) keep fp32's relative accuracy.
 * grad is d sdf / d point in NETWORK coordinates.
 * The trunk is the first 116 slices of the render's packing: `prepacked` is
 * sdfr_render_fc_pack's buffer, the same one sdfr_query_fc_forward takes; NULL packs into
 * the workspace on every call.  The FiLM slots are the render's.
 * sdf (optional) is sdfr_query_fc_forward's SDF bit for bit: the value columns run the
 * same slices in the same k-step order on unscaled inputs.
 * Workspace: 18 KiB of FiLM slots per face + the weight-packing region
 * (sdfr_render_pack_bytes(2)); it does not grow with the point count.  SDFR_EINVAL before
 * any launch for null arguments or required pointers, a null weight pointer (all of
 * sdfr_fc_weights' but sigmoid_beta: packing reads the views layer too), zero sizes, a
 * workspace below sdfr_query_fc_grad_workspace_bytes(B, M), or 2^30 or more padded points
 * B x (M rounded up to 8) in one call (the limit of the query call, kept for both; the
 * size function returns 0 for such a size); SDFR_EUNSUPPORTED for depth != 8 or
 * width != 256.  Asynchronous; allocates nothing.
 * ------------------------------------------------------------------------- */
typedef sdfr_grad_args sdfr_fc_grad_args;    /* prepacked: sdfr_render_fc_pack's buffer */
size_t sdfr_query_fc_grad_workspace_bytes(uint32_t B, uint32_t M);
int sdfr_query_fc_grad(const sdfr_fc_weights *w, const sdfr_fc_grad_args *a, void *stream);

/* ---------------------------------------------------------------------------
 * Surface render (added to ABI 15 without a version step: additive): per camera ray the
 * point where the SDF first changes sign from outside to inside, the unit normal and the
 * field's colour there -- the surface as an image, where the reference's sdf_mesh.py
 * rasterises a marching-cubes or depth mesh with pytorch3d (sdf_utils.py:209-331).  For the
 * ngp and the SIREN network; the two entry points share everything but the weights.
 * The rays and samples z_0..z_{N-1} are those of sdfr_render_*_forward for the same cameras,
 * t_vals, t_rand and sampling flags; sdf_s is the render's return_sdf output bit for bit.
 *   1. Bracket.  s* = the smallest s in [0, N-2] with sdf_s > 0 and sdf_{s+1} <= 0.  None
 *      (N = 1, no sign change, only inside -> outside changes, NaNs) is a miss.  A ray that
 *      starts inside is not special: the samples before its first positive one are skipped,
 *      so the hit is where the ray enters the surface again.  a = z_{s*}, b = z_{s*+1},
 *      fa = sdf_{s*}, fb = sdf_{s*+1}.
 *   2. Refine, K = refine_steps times (a fixed count, no convergence test: nothing is read
 *      back, the call can be captured in a graph): m = fmul(0.5, fadd(a, b)),
 *      p = fadd(o, fmul(d, m)), p_net = fdiv(fmul(p, 2), far - near) under z_normalize, else
 *      p; f = the SDF sdfr_query_*_forward returns at p_net (points in groups of 32, the
 *      SDF does not depend on the group's direction); f > 0: a = m, fa = f, else b = m,
 *      fb = f.
 *   3. Interpolate.  z* = fadd(a, fmul(fdiv(fa, fsub(fa, fb)), fsub(b, a))) clamped to
 *      [a, b] (fa > 0 >= fb); the hit point p* and p*_net by the ops of step 2.
 *   4. Finish.  sdfr_query_*_grad at p*_net gives residual (its SDF there) and g;
 *      e = fdiv(fmul(g, 2), far - near) under z_normalize, else g (the geometry render's
 *      eikonal); normal = e / max(|e|, 1e-20).  sdfr_query_*_forward at p*_net with the
 *      ray's view direction as the render gives it to the network (unit d, or the unit
 *      camera-frame direction under static_viewdirs), one point per direction, gives rgb.
 *   5. A miss: every float map 0, sample -1.
 * Every decision is the sign of an SDF the query call returns, so a caller reproduces the
 * result exactly from the public calls.  Outputs (each may be NULL, one is required; the
 * gradient call runs only for normal / residual, the colour call only for rgb, the bracket
 * and refinement only for a map):
 *   hit [B,1,H,W] 1.0 / 0.0, sample [B,1,H,W] s* or -1, depth [B,1,H,W] z*, residual
 *   [B,1,H,W], xyz [B,3,H,W] p* (world), normal [B,3,H,W], rgb [B,3,H,W] in [0,1],
 *   sdf [B,H,W,N] the coarse SDF.
 * pix_y may be the renderer's buffer offset by y0 with H = a band of rows (W stays the
 * image width), as in sdfr_render_ngp_geometry.
 * Workspace, regions in order, each rounded up to 256 bytes; M = H W, Mp = M rounded up to
 * 32, S = B M N, rays = B M, P = B Mp:
 *   the evaluations' region: ngp sdfr_query_ngp_workspace_bytes(B, 16, Pq / 16) with
 *     Pq = max((M rounded up to 16) N, (Mp / 32 rounded up to 16) 32) padded points per
 *     face; SIREN sdfr_query_siren_workspace_bytes's
 *   the gradient's region: sdfr_query_{ngp,siren}_grad_workspace_bytes(B, M)
 *   sample points [S][3] | (z, dist) [S][2] | coarse sdf [S] (unused when `sdf` is given) |
 *   brackets [rays][4] | s* [rays] | z* [rays] | midpoints [P][3] | their sdf [P] | hit points
 *   [rays][3] | directions [rays][3] | gradient call's sdf [rays] and gradient [rays][3] |
 *   colour call's sdf [rays] and rgb [rays][3]
 * The size functions return 0 for zero sizes and for sizes the underlying calls cannot
 * index: M N, Pq or B Pq at or above 2^25 (ngp) or 2^30 (SIREN).
 * SDFR_EINVAL before any launch for null arguments or required pointers, zero sizes, every
 * output null, refine_steps > 32, a workspace below the size function's value, or too many
 * points; SDFR_EUNSUPPORTED for num_levels != 16 (ngp), depth != 8 or width != 256 (SIREN).
 * sigmoid_beta is not read.  Asynchronous on `stream`; allocates nothing.
 * ------------------------------------------------------------------------- */
typedef struct sdfr_surface_args {
    uint32_t B, H, W, N;              /* faces, image rows, cols, samples per ray           */
    const float *cam, *focal, *near_, *far_, *styles, *pix_x, *pix_y, *t_vals;
    const float *t_rand;              /* as sdfr_ngp_render_args; may be NULL               */
    int t_rand_per_sample, offset_sampling, static_viewdirs, z_normalize;
    uint32_t refine_steps;            /* K, 0..32; 0 = linear interpolation between samples */
    float *hit;  int32_t *sample;     /* [B,1,H,W] 1.0/0.0 ; s* or -1                       */
    float *depth, *residual;          /* [B,1,H,W]                                          */
    float *xyz, *normal, *rgb;        /* [B,3,H,W]                                          */
    float *sdf;                       /* [B,H,W,N] coarse SDF, optional                     */
    void *workspace; size_t workspace_bytes;
    const void *prepacked;            /* sdfr_render_{ngp,siren}_pack's buffer or NULL      */
    const void *prepacked_grad;       /* SIREN: sdfr_query_siren_grad_pack's buffer or NULL; */
                                      /* ngp: ignored                                        */
} sdfr_surface_args;
size_t sdfr_render_ngp_surface_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N);
size_t sdfr_render_siren_surface_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N);
int sdfr_render_ngp_surface(const sdfr_ngp_weights *w, const sdfr_surface_args *a, void *stream);
int sdfr_render_siren_surface(const sdfr_siren_weights *w, const sdfr_surface_args *a,
                              void *stream);

/* Accuracy probe for the two device sin implementations the field kernel can
 * use (software Cody-Waite + polynomial, hardware v_sin_f32 after reduction):
 * out_cw[i] = sin_cw(x[i]), out_hw[i] = sin_hw(x[i]), n elements. */
int sdfr_debug_sin_probe(const float *x, float *out_cw, float *out_hw, uint32_t n,
                         void *stream);

/* Accuracy probe for the split-fp16 field kernel's FiLM sin, whose argument is in
 * revolutions (1/(2 pi) folded into the FiLM vectors): out[i] = sin(2 pi u[i]) by
 * v_fract_f32 + v_sin_f32, n elements. */
int sdfr_debug_sin_rev_probe(const float *u, float *out, uint32_t n, void *stream);

/* Camera parameters from sampled angles (generate_camera_params, sdf_utils.py:97-159,
 * after its random draws; distance 1): viewpoint [B,2] = (azim, elev); ext [B,3,4] =
 * [R^T | T] with T = (cos e sin a, sin e, cos e cos a), R rows = normalize(up x z),
 * normalize(z x x), z = normalize(T), and the degenerate-x replacement of :151-154;
 * near / far [B] = 1 -/+ dist_radius; focal [B] = half_res / tan(fov_ang pi / 180).
 * azim, elev [B] on the device; fp32, one rounding per op. */
int sdfr_camera_extrinsics(const float *azim, const float *elev, uint32_t B, float dist_radius,
                           float fov_ang, float half_res, float *ext, float *focal, float *near_,
                           float *far_, float *viewpoint, void *stream);

/* ---------------------------------------------------------------------------
 * Renderer MLP linear layers for training (no reference native op: they replace
 * the rocBLAS fp32 GEMMs of F.linear in FiLMSiren / LinearLayer, sdf_model.py:23-69,
 * and of their autograd backward, on the op-by-op path stage-1 training takes,
 * training_utils.py:396-451).  Split-fp16 MFMA, fp32 accumulation, fp32-level
 * accuracy (rows / columns scaled by powers of two so no fp16 lo part goes
 * subnormal).  Row-major fp32 tensors; x, out, y_save 16-B aligned, and bias,
 * gamma, beta (read as 16-B vectors) 16-B aligned.
 *
 * sdfr_linear_pack: B [N,K] = w (transposed = 0; w is [N,K]) or w^T (transposed = 1;
 *   w is [K,N]) -> sdfr_linear_pack_bytes(N, K) bytes of split fragments + row scales.
 * sdfr_linear_f16x3: out [M,N] = x [M,K] . B^T (+ bias [N], NULL = none).  Forward
 *   (B = W [N,K]) and input gradient (B = W^T).  Shapes: (N, K) = (256, K <= 32 |
 *   <= 256 | <= 288) or (N <= 32 | <= 256 | <= 272, K <= 256), N and K multiples of 4.
 * sdfr_linear_wgrad_f16x3: gw [N,K] = dy[M,N]^T . x[M,K] (weight gradient), N = 256,
 *   K <= 288; ws >= sdfr_linear_wgrad_ws_bytes(M, N, K).  The sum over M is split
 *   over workgroups and their partials added in a fixed order (deterministic); each
 *   workgroup scales a column by the running maximum of the rows it has read, so
 *   dy and x are each read once (no separate column-maximum pass).
 * ------------------------------------------------------------------------- */
size_t sdfr_linear_pack_bytes(uint32_t N, uint32_t K);
int sdfr_linear_pack(const float *w, uint32_t N, uint32_t K, int transposed, void *packed,
                     void *stream);
int sdfr_linear_f16x3(float *out, const float *x, const void *packed, const float *bias,
                      uint32_t M, uint32_t N, uint32_t K, void *stream);
size_t sdfr_linear_wgrad_ws_bytes(uint32_t M, uint32_t N, uint32_t K);
int sdfr_linear_wgrad_f16x3(float *gw, const float *dy, const float *x, uint32_t M, uint32_t N,
                            uint32_t K, void *ws, size_t ws_bytes, void *stream);

/* FiLMSiren.forward / backward (sdf_model.py:62-67) around the same GEMM, F faces of
 * rows_per_face consecutive rows each (M = F rows_per_face), N = 256:
 * sdfr_film_linear_f16x3: y_save = x . W^T + bias; out = sin(gamma[f] * y + beta[f])
 *   (gamma, beta [F,N]; one rounding per op, as the reference's separate ops).
 * sdfr_film_backward: with u = gamma[f] y + beta[f] recomputed, du = ds cos(u):
 *   dy = du gamma[f] [M,N] (the input of the two GEMM gradients), dgamma[f] = sum du y,
 *   dbeta[f] = sum du, dbf[f] = sum dy (the bias gradient, per face) [F,N] each;
 *   every sum in a fixed order; ws >= sdfr_film_backward_ws_bytes(M, N, rows_per_face). */
int sdfr_film_linear_f16x3(float *out, float *y_save, const float *x, const void *packed,
                           const float *bias, const float *gamma, const float *beta, uint32_t M,
                           uint32_t N, uint32_t K, uint32_t rows_per_face, void *stream);
size_t sdfr_film_backward_ws_bytes(uint32_t M, uint32_t N, uint32_t rows_per_face);
int sdfr_film_backward(float *dy, float *dgamma, float *dbeta, float *dbf, const float *ds,
                       const float *y, const float *gamma, const float *beta, uint32_t M,
                       uint32_t N, uint32_t rows_per_face, void *ws, size_t ws_bytes,
                       void *stream);

/* sdfr_film_backward_grad: the derivative of sdfr_film_backward's (dy, dgamma, dbeta)
 * w.r.t. (ds, y, gamma, beta) -- the second-order step of a FiLM layer whose backward
 * was built with create_graph (the SIREN eikonal term, sdf_model.py:224-229, then
 * differentiated by the loss).  Given the upstream gradients g_dy [M,N], g_dgamma,
 * g_dbeta [F,N] (each may be NULL = 0), with u = gamma[f] y + beta[f] and
 * H = g_dy gamma[f] + g_dgamma[f] y + g_dbeta[f]:
 *   d_ds = H cos u, d_y = -H ds sin u gamma[f] + g_dgamma[f] ds cos u  [M,N],
 *   d_gamma[f] = sum (-H ds sin u y + g_dy ds cos u), d_beta[f] = sum -H ds sin u  [F,N];
 * sums in a fixed order; ws >= sdfr_film_backward_grad_ws_bytes(M, N, rows_per_face). */
size_t sdfr_film_backward_grad_ws_bytes(uint32_t M, uint32_t N, uint32_t rows_per_face);
int sdfr_film_backward_grad(float *d_ds, float *d_y, float *d_gamma, float *d_beta,
                            const float *ds, const float *y, const float *gamma,
                            const float *beta, const float *g_dy, const float *g_dgamma,
                            const float *g_dbeta, uint32_t M, uint32_t N, uint32_t rows_per_face,
                            void *ws, size_t ws_bytes, void *stream);

/* The MLP's narrow output heads for training (sigma_linear 256 -> 1, rgb_linear
 * 256 -> 3; LinearLayer, sdf_model.py:23-41, at :1586-1588), fp32 FMAs, J <= 4 outputs,
 * K <= 256 inputs (a multiple of 4), 16-B aligned x, w, gx:
 * sdfr_linear_head_forward: out [M,J] = x [M,K] . w [J,K]^T (+ bias [J], NULL = none).
 * sdfr_linear_head_backward: gx [M,K] = gy [M,J] . w; gw [J,K] = gy^T . x; gb [J] =
 *   column sums of gy -- each NULL to skip; gw / gb need ws >=
 *   sdfr_linear_head_ws_bytes(M, J, K) (per-workgroup partials added in a fixed order). */
int sdfr_linear_head_forward(float *out, const float *x, const float *w, const float *bias,
                             uint32_t M, uint32_t J, uint32_t K, void *stream);
size_t sdfr_linear_head_ws_bytes(uint32_t M, uint32_t J, uint32_t K);
int sdfr_linear_head_backward(float *gx, float *gw, float *gb, const float *gy, const float *x,
                              const float *w, uint32_t M, uint32_t J, uint32_t K, void *ws,
                              size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * StyleGAN2 decoder ops (im2scene/sdf/models/sdf_op.py).
 *
 * sdfr_fused_bias_act <- fused_bias_act (fused_bias_act.cpp:11,
 *   fused_bias_act_kernel.cu:18; callers sdf_op.py:29, :49, :64):
 *   out[i] = f(x[i] + bias[(i / step_b) % size_b]) * scale over size_x floats,
 *   f by (act, grad): (1,*) identity, (3,0) x>0 ? x : alpha*x,
 *   (3,1) ref[i]>0 ? x : alpha*x, (*,2) 0.  bias NULL (size_b 0) = no bias;
 *   ref may be NULL unless (act, grad) == (3, 1).  out may alias x.
 * ------------------------------------------------------------------------- */
int sdfr_fused_bias_act(float *out, const float *x, const float *bias, const float *ref,
                        uint64_t size_x, uint32_t step_b, uint32_t size_b, int act,
                        int grad, float alpha, float scale, void *stream);

/* sdfr_mapping_linear: one mapping-network layer for inference (sdf_model.py:437-466
 * MappingLinear, EqualLinear + fused_leaky_relu, PixelNorm):
 *   x' = pixelnorm ? x * rsqrt(mean(x^2) + 1e-8) : x           (per sample)
 *   y  = x' . (W * wscale)^T + b * bscale                       (b NULL: no bias)
 *   out = act ? (y > 0 ? y : y * slope) * act_scale : y
 * x [B, K], W [O, K] (16-B aligned), b [O], out [B, O]; K = 256 or 512.
 * fp32 throughout; summation order differs from a GEMM's (fp32 rounding level). */
int sdfr_mapping_linear(float *out, const float *x, const float *w, const float *b, uint32_t B,
                        uint32_t K, uint32_t O, float wscale, float bscale, int act, float slope,
                        float act_scale, int pixelnorm, void *stream);

/* sdfr_decoder_styles: the fused decoder's per-call style prep (sdf_model.py:676-699):
 *   mods[off_k + b c_k + c] = latent[b, idx_k] . mod_w[k, c] + mod_b[k, c]
 *     (mod_w = EqualLinear weight * scale, mod_b = bias * lr_mul; rows zero-padded to cmax)
 *   demods[doff_j + b o_j + o] = rsqrt(dem_eps[j, o] + sum_c mods[layer_j][b, c]^2 dem_w[j, o, c])
 *     (dem_w = su^2 sum_{ky,kx} w^2 transposed to [Cout, Cin], dem_eps = su^2 1e-8).
 * K (style dim) and cmax are 256 or 512; L, J <= 16.  fp32, dot products summed in
 * a fixed order that is not a GEMM's (fp32 rounding level). */
typedef struct sdfr_style_args {
    uint32_t B, n_latent, K;
    const float *latent;              /* [B, n_latent, K]                        */
    uint32_t L, cmax;
    const float *mod_w;               /* [L, cmax, K]                            */
    const float *mod_b;               /* [L, cmax]                               */
    uint32_t mod_index[16], mod_c[16], mod_off[16];
    float *mods;                      /* per layer [B, c_k] at mod_off[k]        */
    uint32_t J, omax;
    const float *dem_w;               /* [J, omax, cmax]                         */
    const float *dem_eps;             /* [J, omax]                               */
    uint32_t dem_layer[16], dem_c[16], dem_off[16];
    float *demods;                    /* per layer [B, o_j] at dem_off[j]        */
} sdfr_style_args;

int sdfr_decoder_styles(const sdfr_style_args *a, void *stream);

/* sdfr_upfirdn2d <- upfirdn2d (upfirdn2d.cpp:12, upfirdn2d_kernel.cu; caller
 * sdf_op.py:230): input viewed as [major, in_h, in_w] (minor = 1), kernel
 * [kernel_h, kernel_w] (device), out [major, out_h, out_w] with
 *   out_h = (in_h*up_y + pad_y0 + pad_y1 - kernel_h) / down_y + 1  (same for w):
 * zero-insertion upsample, pad (negative = crop), true convolution with the
 * kernel, then keep every down-th sample (upfirdn2d_native, sdf_op.py:273). */
int sdfr_upfirdn2d(float *out, const float *input, const float *kernel, uint32_t major,
                   uint32_t in_h, uint32_t in_w, uint32_t kernel_h, uint32_t kernel_w,
                   int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                   int pad_y0, int pad_y1, void *stream);

/* Fused StyledConv / ToRGB epilogue (no reference counterpart: replaces the
 * chain after each decoder convolution -- ModulatedConv2d demodulation and
 * upsample blur (sdf_model.py:676-699), NoiseInjection (:704), FusedLeakyReLU
 * (:818), ToRGB + skip Upsample (:821-843) -- with one pass over the
 * activations).  Activations are NHWC (channels_last):
 *   conv  [B,H,W,C], or [B,2H+1,2W+1,C] when blur_up (stride-2 transposed conv
 *         output; blurred with outer(fir,fir), pad (1,1), as ModulatedConv2d.blur)
 *   v     = lrelu((blur(conv) * demod[b,c] + noise_weight * noise[b,h,w])
 *                 + bias[c], negative_slope) * act_scale
 *   y     [B,H,W,C] = v * s_next[b,c] (the next conv's modulation; s_next NULL
 *         -> v), or y NULL (not stored)
 *   rgb   [B,3,H,W] (NCHW) = sum_c v * rgb_w[b,o,c] + rgb_b[o]
 *         + upfirdn2d(skip, outer(fir,fir), up 2, pad (2,1)) when skip != NULL;
 *         only when rgb_w != NULL, and not together with blur_up.
 * C must be a multiple of 4; with rgb_w, C/4 must be a power of two <= 64 or
 * a multiple of 64 (C <= 1024). */
typedef struct sdfr_styled_epilogue_args {
    uint32_t B, C, H, W;
    const float *conv;
    int blur_up;
    float fir[4];                 /* separable taps; outer(fir,fir) = the 2-D kernel */
    const float *demod;           /* [B,C] or NULL (no demodulation)               */
    const float *noise;           /* [B,H,W] or NULL                               */
    const float *noise_weight;    /* [1] NoiseInjection.weight (device)            */
    const float *bias;            /* [C] FusedLeakyReLU.bias                       */
    float negative_slope, act_scale;
    const float *s_next;          /* [B,C] or NULL                                 */
    float *y;                     /* [B,H,W,C] or NULL                             */
    const float *rgb_w;           /* [B,3,C] modulated ToRGB weight or NULL        */
    const float *rgb_b;           /* [3]                                           */
    const float *skip;            /* [B,3,H/2,W/2] or NULL                         */
    float *rgb;                   /* [B,3,H,W]                                     */
    /* instead of y: the round-to-nearest fp16 split y = hi + lo in the split-NHWC
     * layout below (the input format of sdfr_conv3x3_f16x3), or NULL */
    void *y_split;
} sdfr_styled_epilogue_args;

int sdfr_styled_epilogue(const sdfr_styled_epilogue_args *a, void *stream);

/* Decoder input staging: y[b,h,w,c] = x[b,c,h,w] * s[b,c] (NCHW -> NHWC with
 * the first ModulatedConv2d's modulation folded in).  C and H*W multiples of 4. */
int sdfr_modulate_to_nhwc(float *y, const float *x, const float *s, uint32_t B, uint32_t C,
                          uint32_t HW, void *stream);
/* The same with y written in the split-NHWC layout (C % 8 == 0).
 *
 * Split-NHWC: the round-to-nearest fp16 split x = hi + lo of an NHWC fp32 tensor,
 * fp16 [B,H,W,C/8,2,8]: per pixel and group of 8 channels, 8 hi then 8 lo
 * halves (32 channels of one pixel = one 128-B line). */
int sdfr_modulate_to_nhwc_split(void *y_split, const float *x, const float *s, uint32_t B,
                                uint32_t C, uint32_t HW, void *stream);

/* ---------------------------------------------------------------------------
 * Decoder 3x3 convolutions on split-fp16 MFMA (no reference counterpart: they
 * replace the MIOpen convolutions of ModulatedConv2d on the fused decoder path,
 * sdf_model.py:676-699, batched form conv(x * s, w) * demod).
 *
 * sdfr_conv_pack_weights: w [Cout][Cin][3][3] (ModulatedConv2d.weight[0]) times
 *   scale -> su [Cout] (per-row power-of-two scale, written) and the packed hi/lo
 *   fp16 fragments (sdfr_conv_pack_bytes(Cout, Cin) - 4*Cout bytes).
 * sdfr_conv3x3_f16x3: input in the split-NHWC layout ([B,H,W,Cin/8,2,8] fp16, as
 *   written by the *_split / y_split outputs above), NHWC fp32 out, result
 *   multiplied by su[o]
 *   (the caller folds 1/su into the demodulation -- exact, powers of two):
 *   transposed = 0: out [B,H,W,Cout] = conv2d(x, w, padding 1);
 *   transposed = 1: out [B,2H+1,2W+1,Cout] = conv_transpose2d(x, w^T, stride 2)
 *   (x [B,H,W,Cin]).  Cout % 128 == 0, Cin % 32 == 0.
 * ------------------------------------------------------------------------- */
size_t sdfr_conv_pack_bytes(uint32_t Cout, uint32_t Cin);
int sdfr_conv_pack_weights(const float *w, float scale, uint32_t Cout, uint32_t Cin,
                           void *packed, float *su, void *stream);
int sdfr_conv3x3_f16x3(float *out, const void *x_split, const void *packed,
                       uint32_t B, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout,
                       int transposed, void *stream);
/* The same with a workspace: when the grid would leave CUs idle (small batches,
 * e.g. eval.py's one face) the K-steps of every tile are shared by 2-4 workgroups
 * whose fp32 partial tiles a second kernel sums in a fixed order (deterministic).
 * ws_bytes >= sdfr_conv_ws_bytes(B, H, W, Cout, transposed) enables it (0: no split
 * for this shape; a smaller or NULL workspace runs unsplit).  The size is the one from
 * which the launch plan (sdfr_conv_plan below) takes its split, under the current conv_t
 * mode. */
int sdfr_conv3x3_f16x3_ws(float *out, const void *x_split, const void *packed,
                          uint32_t B, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout,
                          int transposed, void *ws, size_t ws_bytes, void *stream);
size_t sdfr_conv_ws_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t Cout, int transposed);
/* Which kernel runs the transposed convolution (a process-wide setting, read by both
 * the launch and sdfr_conv_ws_bytes, so they always agree): 1 (default) conv_t_kernel
 * from 256 tiles of 64 channels x 16 x 16 positions, conv_x_kernel's split-K below;
 * 0 always conv_x_kernel; 2 conv_t_kernel at any tile count; 3 as 2 with each tile's
 * channel groups split 2 or 4 ways below 256 tiles (needs the workspace).  The
 * initial value is SDFR_CONV_T from the environment when the library loads (else 1);
 * mode -1 restores it.  Returns the previous mode, or SDFR_EINVAL for another value. */
int sdfr_set_conv_t_mode(int mode);

/* The regular (transposed = 0) convolution with the plain styled epilogue fused
 * into it (the conv output never goes to memory): per pixel and channel
 *   v = lrelu((conv * demod[b,c] + noise_weight * noise[b,h,w]) + bias[c],
 *             negative_slope) * act_scale         (demod already divided by su)
 *   y_split = v * s_next[b,c] in split-NHWC (s_next NULL -> v), when y_split
 *   rgb_partial[k,b,o,h,w] = sum_{c in [128k, 128k+128)} v * rgb_w[b,o,c], when
 *   rgb_w (k < Cout/128; sdfr_rgb_finish adds the parts, bias and skip); or, with
 *   rgb_base instead of rgb_w, rgb_w[b,o,c] = rgb_base[o,c] * rgb_s[b,c] (fp32 product
 *   formed in the kernel: ToRGB's scaled 1x1 weight times the face's style, the
 *   caller's [B,3,Cout] multiply saved).
 * Same operation order as sdfr_styled_epilogue for v and y.  H*W % 256 == 0. */
typedef struct sdfr_conv_act_args {
    const void *x_split;          /* [B,H,W,Cin/8,2,8] fp16                         */
    const void *packed;           /* sdfr_conv_pack_weights                         */
    uint32_t B, H, W, Cin, Cout;
    const float *demod;           /* [B,Cout]                                       */
    const float *noise;           /* [B,H,W] or NULL                                */
    const float *noise_weight;    /* [1] (device)                                   */
    const float *bias;            /* [Cout]                                         */
    float negative_slope, act_scale;
    const float *s_next;          /* [B,Cout] or NULL                               */
    void *y_split;                /* [B,H,W,Cout/8,2,8] fp16 or NULL                */
    const float *rgb_w;           /* [B,3,Cout] modulated ToRGB weight or NULL      */
    float *rgb_partial;           /* [Cout/128,B,3,H,W] fp32 (with rgb_w)           */
    void *ws;                     /* split-K partials or NULL                       */
    size_t ws_bytes;              /* >= sdfr_conv_act_ws_bytes(...) to split        */
    const float *rgb_base;        /* [3,Cout] (rgb_w NULL) or NULL         (ABI 10) */
    const float *rgb_s;           /* [B,Cout] with rgb_base                (ABI 10) */
} sdfr_conv_act_args;

int sdfr_conv3x3_f16x3_act(const sdfr_conv_act_args *a, void *stream);
/* Workspace that lets sdfr_conv3x3_f16x3_act split K when B*H*W/256 * Cout/128
 * workgroups would leave CUs idle (0: no split for this shape): the K-steps are
 * shared by 2 or 4 workgroups per tile, whose fp32 partial tiles a second kernel
 * sums in a fixed order before the epilogue. */
size_t sdfr_conv_act_ws_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t Cout);

/* The upsampling StyledConv in one call (ABI 13; sdf_model.py:660-701 + 704-818):
 * conv_transpose2d(x, w^T, stride 2) (the packed weights as sdfr_conv3x3_f16x3),
 * Blur(outer(fir, fir), pad (1, 1)) down to 2H x 2W, then per pixel and channel
 *   v = lrelu(blur * demod[b,o] + noise_weight * noise[b,y,x] + bias[o]) * act_scale
 * and y_split = split-NHWC fp16 of v * s_next[b,o] (sdfr_styled_epilogue's blur_up
 * arithmetic, in its order: the same bits as sdfr_conv3x3_f16x3 + that epilogue).
 * The blur and epilogue run inside the conv kernel for each block's interior pixels;
 * `raw` [B,2H+1,2W+1,Cout] fp32 is a workspace that receives only the conv values
 * of the blocks' band rows / columns, from which a second kernel finishes the block
 * border pixels.  Needs sdfr_conv_t_act_supported (H, W % 16 == 0 and at least 256
 * tiles of 64 channels x 16 x 16 positions; SDFR_EUNSUPPORTED otherwise). */
typedef struct sdfr_conv_t_act_args {
    const void *x_split;          /* [B,H,W,Cin/8,2,8] fp16                         */
    const void *packed;           /* sdfr_conv_pack_weights                         */
    uint32_t B, H, W, Cin, Cout;  /* input H x W; output 2H x 2W                    */
    float fir[4];                 /* the blur's 1-D taps                            */
    const float *demod;           /* [B,Cout] (x 1/su)                              */
    const float *noise;           /* [B,2H,2W] or NULL                              */
    const float *noise_weight;    /* [1] (device)                                   */
    const float *bias;            /* [Cout]                                         */
    float negative_slope, act_scale;
    const float *s_next;          /* [B,Cout] or NULL                               */
    void *y_split;                /* [B,2H,2W,Cout/8,2,8] fp16                      */
    float *raw;                   /* [B,2H+1,2W+1,Cout] fp32 workspace              */
} sdfr_conv_t_act_args;
int sdfr_conv_t_act(const sdfr_conv_t_act_args *a, void *stream);
int sdfr_conv_t_act_supported(uint32_t B, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout);

/* The launch plan of one decoder convolution under the current conv_t mode, as the three
 * entry points above would run it: which kernels, with which grids, after which refusal.
 * Host arithmetic only (no HIP call, no launch), so tests can pin the dispatch without a
 * GPU.  Returns info->rc: SDFR_OK, or the code the entry point would refuse the shape
 * with (sdfr_last_error() then holds the reason); SDFR_EINVAL for null arguments. */
enum { SDFR_CONV_EPI_RAW = 0,      /* sdfr_conv3x3_f16x3[_ws]                        */
       SDFR_CONV_EPI_STYLED = 1,   /* sdfr_conv3x3_f16x3_act (transposed = 0)        */
       SDFR_CONV_EPI_BLUR = 2 };   /* sdfr_conv_t_act        (transposed = 1)        */
enum { SDFR_CONV_K_X = 0,          /* conv_x_kernel<false>                           */
       SDFR_CONV_K_X_ACT,          /* conv_x_kernel<true>                            */
       SDFR_CONV_K_SPLITK,         /* conv_splitk_kernel<false>                      */
       SDFR_CONV_K_SPLITK_ACT,     /* conv_splitk_kernel<true>                       */
       SDFR_CONV_K_H,              /* conv_h_kernel<false>                           */
       SDFR_CONV_K_H_SPLIT,        /* conv_h_kernel<true>                            */
       SDFR_CONV_K_H_FINISH,       /* conv_h_finish_kernel                           */
       SDFR_CONV_K_T,              /* conv_t_kernel<false>                           */
       SDFR_CONV_K_T_FUSE,         /* conv_t_kernel<true>                            */
       SDFR_CONV_K_T_FINISH,       /* conv_t_finish_kernel                           */
       SDFR_CONV_K_T_BORDER_ROWS,  /* conv_t_border_kernel<true>                     */
       SDFR_CONV_K_T_BORDER_COLS };/* conv_t_border_kernel<false>                    */
#define SDFR_CONV_PLAN_MAX_STEPS 6
typedef struct sdfr_conv_plan_query {
    uint32_t B, H, W, Cin, Cout;  /* input H x W                                    */
    int transposed;
    int epilogue;                 /* SDFR_CONV_EPI_*                                */
    int has_ws;                   /* a workspace is offered ...                     */
    size_t ws_bytes;              /* ... of this size                               */
} sdfr_conv_plan_query;
typedef struct sdfr_conv_plan_info {
    int rc;
    uint32_t ksplit;              /* split-K factor of conv_x_kernel / conv_h_kernel */
    uint32_t ksplit_t;            /* channel-group split of conv_t_kernel's tiles   */
    size_t ws_bytes;              /* workspace from which the path takes its split  */
    uint32_t nsteps;
    struct { uint32_t kernel, grid_x, grid_y, block; } steps[SDFR_CONV_PLAN_MAX_STEPS];
} sdfr_conv_plan_info;
int sdfr_conv_plan(const sdfr_conv_plan_query *q, sdfr_conv_plan_info *info);

/* ToRGB finish: rgb [B,3,H,W] = sum_k partial[k] + rgb_b[o]
 *   + upfirdn2d(skip, outer(fir,fir), up 2, pad (2,1)) when skip != NULL
 * (partial [nparts,B,3,H,W], skip [B,3,H/2,W/2], fir: 4 host floats). */
int sdfr_rgb_finish(float *rgb, const float *partial, uint32_t nparts, const float *rgb_b,
                    const float *skip, const float *fir, uint32_t B, uint32_t H, uint32_t W,
                    void *stream);

/* ---------------------------------------------------------------------------
 * Marching cubes (sdf_mesh.py's surface extraction: sdf_utils.py:188-205, which
 * calls scikit-image's marching_cubes(sdf_vol, 0) on the host; csrc/mesh.hip).
 *
 * Volume: n0 x n1 x n2 fp32 points (each >= 2, 4 n0 n1 n2 + 1 < 2^32) on the
 * device, point (i, j, k) at vol[i s0 + j s1 + k s2] (element strides, so the
 * reference's permute(1, 0, 2) is a stride swap).  A corner is inside when its
 * value < level; vertices lie on the sign-changing grid edges by linear
 * interpolation, in index coordinates (x = i + t ...).
 *
 *   sdfr_mc_count:  classify + scan into ws; writes counts[0] = vertices,
 *                   counts[1] = triangles to HOST memory (synchronises stream)
 *   sdfr_mc_emit:   same volume and ws (after sdfr_mc_count): verts [V,3] fp32,
 *                   faces [F,3] int32 (vertex ids), device
 * ------------------------------------------------------------------------- */
size_t sdfr_mc_workspace_bytes(uint32_t n0, uint32_t n1, uint32_t n2);
int sdfr_mc_count(const float *vol, uint32_t n0, uint32_t n1, uint32_t n2, int64_t s0,
                  int64_t s1, int64_t s2, float level, void *ws, size_t ws_bytes,
                  uint32_t *counts, void *stream);
int sdfr_mc_emit(const float *vol, uint32_t n0, uint32_t n1, uint32_t n2, int64_t s0,
                 int64_t s1, int64_t s2, float level, const void *ws, size_t ws_bytes,
                 float *verts, int32_t *faces, void *stream);

/* ---------------------------------------------------------------------------
 * Sparse marching cubes: narrow-band SDF bricks (csrc/mesh_sparse.hip).
 *
 * Grid and bricks.  The grid has res points per axis, res a multiple of 8; a point
 * has index (ix, iy, iz), a cell its low corner at ix, iy, iz <= res - 2.  A brick
 * is 8 x 8 x 8 points; nb = res / 8 bricks per axis (1 <= nb <= 256), brick
 * (bx, by, bz) has linear index q = (bx nb + by) nb + bz.  A cell belongs to the
 * brick of its low corner, so the cells of brick K read points of K + {0,1}^3.
 * Storage: values [n, 8, 8, 8] fp32 (local lx, ly, lz; lz fastest), a slot table
 * slots [nb^3] int32 (slot, or -1) and surface [nb^3] uint8 (the bricks whose
 * cells are triangulated).  A point is inside when v < level, as in the dense code.
 *
 * Layout.  A brick is needed when it lies in K + {0,1}^3 (clipped to the grid) of
 * some surface brick K.  Needed bricks without a slot get the slots n_prev,
 * n_prev + 1, ... in ascending q; existing slots never move.
 *
 * Mesh.  The cells of surface bricks are triangulated with mc_table.h; a vertex
 * sits on each crossed grid edge by the dense code's arithmetic (low end +
 * fdiv(fsub(level, va), fsub(vb, va))), in global index coordinates, and only on
 * an edge that an emitted triangle references (an edge of a surface brick's
 * cell): no unreferenced vertices.  Vertices are shared between cells and across
 * brick borders as in the dense mesh, which the result equals, as a set of
 * triangles, on the cells of surface bricks.  Order is a pure function of slots
 * and values: slot-major; within a brick vertices axis-major then local point
 * order, triangles in local cell order then table order.
 *
 * Leaks.  For a cell of surface brick K and one of its faces whose cell across
 * exists and lies in a brick K' that is not surface: if the face's four corners
 * are not all on the same side of level, grow[K'] = 1.  Growth (the caller's
 * loop): surface |= grow, layout, evaluate the new slots, count again, until grow
 * is all zero; the final surface set is the closure of the first one under leaks.
 *
 *   sdfr_brick_layout:  dilates surface to the needed bricks and assigns the new
 *                       slots (ws: sdfr_brick_layout_workspace_bytes(nb)); writes
 *                       the number of slots now in use to HOST memory *n_total
 *                       (synchronises stream).  slots starts as all -1, n_prev 0.
 *   sdfr_brick_points:  points [(slot1 - slot0) 512, 3] of the bricks with a slot in
 *                       [slot0, slot1), brick-major in slot order: point
 *                       (ix, iy, iz) is (ax[ix], ay[iy], az[iz]), ax / ay / az [res]
 *                       fp32 tables (entries are copied, nothing is computed).
 *   sdfr_mc_sparse_count: classify + scan into ws
 *                       (sdfr_mc_sparse_workspace_bytes(n_bricks): 16 bytes per
 *                       stored point + 4 per brick + the scan's block sums);
 *                       n_bricks = the layout's n_total, every slot's values
 *                       filled.  grow [nb^3] uint8 or NULL: cleared, then set to 1
 *                       per the leak rule with plain stores.  counts[0] = vertices,
 *                       counts[1] = triangles to HOST memory (synchronises stream).
 *   sdfr_mc_sparse_emit: same arguments and ws (after the count): verts [V,3] fp32,
 *                       faces [F,3] int32 (vertex ids), device.
 *
 * SDFR_EINVAL before any launch for null pointers (grow excepted), nb == 0 or
 * nb > 256, n_bricks == 0, 4 * 512 n_bricks + 1 >= 2^32 (the size function
 * returns 0 for such a count), a short workspace, slot0 >= slot1.  Table entries
 * are bounds-checked on the device: a slot outside [0, n_bricks) reads as NaN.
 * Everything but the two host reads is asynchronous on stream; nothing allocates.
 * ------------------------------------------------------------------------- */
size_t sdfr_brick_layout_workspace_bytes(uint32_t nb);
int sdfr_brick_layout(const uint8_t *surface, uint32_t nb, int32_t *slots, uint32_t n_prev,
                      void *ws, size_t ws_bytes, uint32_t *n_total, void *stream);
int sdfr_brick_points(const int32_t *slots, uint32_t nb, uint32_t slot0, uint32_t slot1,
                      const float *ax, const float *ay, const float *az, float *points,
                      void *stream);
size_t sdfr_mc_sparse_workspace_bytes(uint32_t n_bricks);
int sdfr_mc_sparse_count(const float *values, const int32_t *slots, const uint8_t *surface,
                         uint32_t nb, uint32_t n_bricks, float level, void *ws, size_t ws_bytes,
                         uint8_t *grow, uint32_t *counts, void *stream);
int sdfr_mc_sparse_emit(const float *values, const int32_t *slots, const uint8_t *surface,
                        uint32_t nb, uint32_t n_bricks, float level, const void *ws,
                        size_t ws_bytes, float *verts, int32_t *faces, void *stream);

/* ---------------------------------------------------------------------------
 * Mesh connected components (added to ABI 15 without a version step: additive;
 * csrc/mesh_cc.hip): label, measure, keep, compact -- where users of the reference call
 * trimesh's mesh.split() on the host and keep the big piece.
 *
 * Mesh: faces [F,3] int32 (F may be 0) over V vertices, verts [V,3] fp32, device.
 * 1 <= V < 2^31 and 3 F < 2^31.  Two vertices are connected when a face references both;
 * a vertex no face references is a component of its own with 0 faces.
 *
 *   sdfr_mesh_cc_label:  lock-free union-find over the face edges (every hook puts the
 *                       larger root under the smaller), then a flatten pass: label[v] =
 *                       the SMALLEST vertex index of v's component -- a pure function of
 *                       the mesh, whatever the scheduling.  comp[v] = the dense id of that
 *                       component: ids 0..C-1 in increasing order of the smallest vertex.
 *                       C goes to HOST memory *n_components (synchronises stream).
 *   sdfr_mesh_cc_stats:  per component (C = the label call's count, comp its output):
 *                       n_vertices, n_faces [C] uint32; bbox [C,6] fp32 = min x y z, max
 *                       x y z over the component's vertices; area_q [C] uint64, the sum of
 *                       the faces' areas in units of *area_unit (HOST; synchronises).
 *                       Integer atomics only: every output is reproducible bit for bit.
 *                       Unit: with d the largest edge of the mesh's bounding box and
 *                       x = 2 d^2 max(F, 1), u = 2^(k - 61), k = the exponent frexp(x)
 *                       gives (x <= 2^k < 2 x); u = 1 when x is 0 or not finite.  A face's
 *                       area, 0.5 |(b - a) x (c - a)| in fp64 from the fp32 vertices, is
 *                       divided by u and rounded to nearest; no sum can reach 2^62.
 *                       |area_q[c] u - exact| <= n_faces[c] u / 2 + 2^11 u (the second
 *                       term covers the fp64 evaluation over the whole mesh).
 *   sdfr_mesh_cc_select_count: keep [C] uint8 (device).  A face is kept when
 *                       keep[comp[its first vertex]]; a vertex when keep[comp[v]] and,
 *                       with drop_unreferenced != 0, a kept face references it.  Flags
 *                       and their scans go into ws; counts[0] = kept vertices, counts[1] =
 *                       kept faces to HOST memory (synchronises stream).
 *   sdfr_mesh_cc_select_emit: same mesh and ws (after the count), V_out / F_out the counts:
 *                       verts_out [V_out,3], faces_out [F_out,3] int32 reindexed,
 *                       index_map [V_out] int32 (new -> old vertex).  Kept vertices and
 *                       kept faces keep their original relative order.
 *
 * ws: sdfr_mesh_cc_workspace_bytes(V, F) bytes for every call (4 bytes per vertex and
 * per face + the scans' block sums + 1 KB; 0 for sizes outside the limits above).
 * SDFR_EINVAL before any launch, nothing written, for null pointers (faces may be null
 * when F is 0), V == 0, V or 3 F >= 2^31, a short workspace, C outside [1, V], V_out
 * outside [1, V] or F_out > F.  A face index outside [0, V) (or a comp entry outside
 * [0, C)) is never dereferenced: the kernels skip the element and set a device error word,
 * which the three synchronising calls read with their counts and return as SDFR_EINVAL
 * (device outputs are then unspecified, *n_components / counts / *area_unit unwritten).
 * Everything but those host reads is asynchronous on stream; nothing allocates.
 * ------------------------------------------------------------------------- */
size_t sdfr_mesh_cc_workspace_bytes(uint32_t V, uint32_t F);
int sdfr_mesh_cc_label(const int32_t *faces, uint32_t V, uint32_t F, int32_t *label,
                       int32_t *comp, void *ws, size_t ws_bytes, uint32_t *n_components,
                       void *stream);
int sdfr_mesh_cc_stats(const float *verts, const int32_t *faces, const int32_t *comp,
                       uint32_t V, uint32_t F, uint32_t C, uint32_t *n_vertices,
                       uint32_t *n_faces, float *bbox, uint64_t *area_q, double *area_unit,
                       void *ws, size_t ws_bytes, void *stream);
int sdfr_mesh_cc_select_count(const int32_t *faces, const int32_t *comp, const uint8_t *keep,
                              uint32_t V, uint32_t F, uint32_t C, int drop_unreferenced,
                              void *ws, size_t ws_bytes, uint32_t *counts, void *stream);
int sdfr_mesh_cc_select_emit(const float *verts, const int32_t *faces, uint32_t V, uint32_t F,
                             uint32_t V_out, uint32_t F_out, const void *ws, size_t ws_bytes,
                             float *verts_out, int32_t *faces_out, int32_t *index_map,
                             void *stream);

/* ---------------------------------------------------------------------------
 * Mesh simplification (added to ABI 15 without a version step: additive;
 * csrc/mesh_simplify.hip): vertex clustering on a uniform grid -- where users of the
 * reference decimate with trimesh on the host.  All vertices of one grid cell become one
 * vertex at their (quantised) mean; faces are remapped, collapsed ones dropped, duplicates
 * removed.  Every output is a pure function of the mesh and the grid (integer atomics only),
 * so a NumPy transcription (tests/mesh_simplify_ref.py) gives the same bits.
 *
 * Inputs.  verts [V,3] fp32 and faces [F,3] int32 on the device, 1 <= V < 2^31,
 * 3 F < 2^31, F may be 0.  Grid: origin (ox, oy, oz) fp32 (finite), cell edge `cell` fp32
 * (finite, > 0), nx, ny, nz each in [1, 2^21] (a cell key fits 63 bits).  Every
 * floating-point step below is one rounded IEEE operation (round to nearest even, nothing
 * contracted).
 *
 * Cell of a vertex, per axis k:  t_k = (v_k - o_k) / cell (one fp32 subtract, one correctly
 * rounded fp32 divide);  c_k = clamp(floor(t_k), 0, n_k - 1), clamped as float before the
 * conversion, so a vertex outside the grid belongs to the nearest boundary cell;
 * key = (c_x ny + c_y) nz + c_z in 64 bits.  A non-finite coordinate is an error.
 *
 * Clusters.  A cluster is the set of vertices with one key; every vertex takes part,
 * referenced by a face or not.  rep = the cluster's smallest vertex index; clusters are
 * numbered 0..C-1 in increasing order of rep.
 *
 * Position of a cluster, per axis:  r_k = clamp(t_k - (float)c_k, 0, 1) in fp32;
 * q_k = (int64) rint(r_k 2^20) (the product is exact);  S_k = sum of q_k over the members
 * in int64 (< 2^52 for any V), m = the member count;
 *   p_k = (float)( (double)o_k + ((double)c_k + (double)S_k / ((double)m 2^20)) (double)cell )
 * with each fp64 operation rounded once and c_k the cell of rep.
 *
 * Faces.  Each corner is mapped to its cluster.  A face with two equal corners is dropped.
 * Two surviving faces with the same vertex SET (any corner order, either orientation) are
 * duplicates: of a class of duplicates the face with the smallest original index is kept,
 * with its own corner order.  Kept faces keep their original relative order.
 *
 * Vertices out.  With drop_unreferenced != 0 a cluster that no kept face references is
 * dropped, otherwise all C are kept; kept clusters are renumbered densely in the same order.
 *
 * Not promised: manifoldness (clustering can pinch a thin part into a non-manifold edge or
 * vertex) and feature preservation (the mean pulls a convex surface inwards, by less than
 * one cell).  Guaranteed for vertices inside the grid: a vertex and its cluster's position
 * lie in one cell, so they differ by at most `cell` per axis.
 *
 *   sdfr_mesh_simplify_count: everything up to the scans, into ws; counts [3] in HOST
 *                       memory = C, V_out, F_out (synchronises stream).
 *   sdfr_mesh_simplify_emit:  same mesh and ws (after the count; the grid is kept in ws),
 *                       V_out / F_out the counts: verts_out [V_out,3], faces_out [F_out,3]
 *                       int32, index_map [V_out] int32 (new vertex -> rep, an old vertex: the
 *                       map that carries attributes), cluster [V] int32 (old vertex -> new
 *                       vertex, or -1 when its cluster was dropped; may be null), members
 *                       [V_out] uint32 (may be null).
 *
 * ws: sdfr_mesh_simplify_workspace_bytes(V, F) bytes, a function of V and F only (two
 * hash tables of the powers of two >= 2 V and >= 2 F slots of 12 and 4 bytes, 44 bytes per
 * vertex, 8 per face, the scans' block sums; 0 for sizes outside the limits).
 * SDFR_EINVAL before any launch, nothing written, for null pointers (faces may be null
 * when F is 0; cluster and members may be null), V or F outside the limits, cell not finite
 * or <= 0, a non-finite origin, a dimension outside [1, 2^21], a short workspace, V_out
 * outside [1, V] or F_out > F.  A face index outside [0, V) or a non-finite vertex
 * coordinate is never used to address memory: the kernels skip the element and set a device
 * error word, which the count call reads with its counts and returns as SDFR_EINVAL
 * ("... outside [0, V)" / "... not finite"; counts unwritten).  Everything but that read is
 * asynchronous on stream; nothing allocates.
 * ------------------------------------------------------------------------- */
size_t sdfr_mesh_simplify_workspace_bytes(uint32_t V, uint32_t F);
int sdfr_mesh_simplify_count(const float *verts, const int32_t *faces, uint32_t V, uint32_t F,
                             float ox, float oy, float oz, float cell,
                             uint32_t nx, uint32_t ny, uint32_t nz, int drop_unreferenced,
                             void *ws, size_t ws_bytes, uint32_t *counts, void *stream);
int sdfr_mesh_simplify_emit(const float *verts, const int32_t *faces, uint32_t V, uint32_t F,
                            uint32_t V_out, uint32_t F_out, const void *ws, size_t ws_bytes,
                            float *verts_out, int32_t *faces_out, int32_t *index_map,
                            int32_t *cluster, uint32_t *members, void *stream);

/* ---------------------------------------------------------------------------
 * Mesh smoothing (added to ABI 15 without a version step: additive;
 * csrc/mesh_smooth.hip): Laplacian and Taubin lambda | mu passes of the uniform umbrella
 * operator on an indexed triangle mesh -- where users of the reference call trimesh's
 * filter_laplacian / filter_taubin on the host.  Floating-point sums over a vertex's
 * neighbours would depend on their order, so the state of the smoothing is integer: every
 * output is a pure function of the mesh, the lattice and the weights, and a NumPy
 * transcription (tests/mesh_smooth_ref.py) gives the same bits.
 *
 * Inputs.  verts [V,3] fp32 and faces [F,3] int32 on the device, 1 <= V < 2^31,
 * 3 F < 2^31, F may be 0.
 *
 * Lattice.  Origin (ox, oy, oz) fp32 (finite) and unit_log2 in [-126, 96]: the unit
 * u = 2^unit_log2 is a normal fp32 and 2^31 u is finite in fp32.  Per vertex and axis
 * q = (int64) rint(((double)v - (double)o) / u): one fp64 subtraction, an exact scaling,
 * ties to even.  Every input q must lie in [0, 2^30]; a vertex outside the lattice or a
 * non-finite coordinate is an error, not clamped.
 *
 * Valence.  d_i = the number of face corners equal to i (a face that lists i twice counts
 * twice).
 *
 * Boundary.  The edge slots of a face (c0, c1, c2) are {c0,c1}, {c1,c2}, {c2,c0}; slots with
 * equal ends are ignored.  The multiplicity of an unordered pair is the number of slots, over
 * all faces, that equal it.  A vertex is a boundary vertex when it is an end of a pair of
 * multiplicity exactly 1 (non-manifold pairs, 3 and more, do not make a boundary).
 *
 * Movable.  d_i > 0 and not (pin_boundary and boundary).
 *
 * One pass of weight w = (double)weight_p (fp32, finite, |w| <= 1), a Jacobi pass: every read
 * is from the previous pass's state.  For every movable i and every axis:
 *   S = the sum, over the corners equal to i, of q[a] + q[b], a and b that face's other two
 *       corners as written (int64, exact);
 *   D = S - 2 d_i q[i] (exact);
 *   q'[i] = clamp(q[i] + (int64) rint((w (double)D) / (double)(2 d_i)), -2^30, 2^31 - 1)
 * -- one fp64 conversion, one product, one quotient, rint with ties to even.  The clamp is a
 * guard that never acts on a sane mesh (one bounding-box extent of slack on either side); it
 * keeps the state in int32, and with it |S| <= 2 d_i (2^31 - 1) and |D| < 3 d_i 2^31: S fits
 * int64 for every permitted mesh (d_i <= 3 F < 2^31), D for d_i <= 2^30.  A vertex with more
 * than 2^30 corners (over 4 GiB of faces on one vertex) is outside the definition.  On a
 * closed manifold this is the uniform umbrella operator (each neighbour is counted twice).
 *
 * Output.  A vertex that was never movable keeps its input coordinates bit for bit, and so
 * does every vertex after 0 passes.  Every other vertex:
 *   p = (float)((double)o + (double)q u)
 * (the product is exact; one fp64 sum, one rounding to fp32).  Faces are not touched.
 *
 * Schedule.  The run call takes a plain array of weights: Laplacian with n iterations is n
 * passes of weight lambda, Taubin n times (lambda, mu), 2 n passes.
 *
 *   sdfr_mesh_smooth_prepare: what all passes share, into ws (the quantised state, every
 *                       vertex's row of neighbours, the movable flags, the lattice); valence
 *                       [V] int32 and boundary [V] uint8 (0 / 1) are device outputs, either
 *                       may be null.  Reads the device error word (synchronises stream).
 *   sdfr_mesh_smooth_run:     same verts, V and ws (after a prepare that returned SDFR_OK);
 *                       weights [n_passes] fp32 in HOST memory, 0 <= n_passes <= 1024 (null
 *                       allowed when 0); verts_out [V,3] fp32, which must not overlap verts.
 *                       Asynchronous on stream.  May be called repeatedly after one prepare:
 *                       each call starts from the prepared state.
 *
 * ws: sdfr_mesh_smooth_workspace_bytes(V, F) bytes, a function of V and F only.  With
 * up(x) = x rounded up to a multiple of 256, Ce = the power of two >= max(4 F, 1) and
 * nb = ceil(V / 2048):
 *   up(4 (V + 1)) + up(4 V) + up(V) + 256 + 3 up(16 V) + up(4 nb + 4) + up(24 F) + up(4 Ce)
 *   + up(8 Ce)
 * (57 bytes per vertex, 24 per face, 12 per edge-table slot; 0 for sizes outside the limits).
 * Both calls return SDFR_EINVAL before any launch, nothing written, for null pointers (faces
 * may be null when F is 0), V or F outside the limits, a short workspace, a non-finite
 * origin, unit_log2 outside [-126, 96], a weight that is not finite or has |w| > 1,
 * n_passes > 1024, or verts_out overlapping verts.  run is not given F: what it reads is laid
 * out at offsets that depend on V alone, the rows after the rest, and it rejects a workspace
 * shorter than sdfr_mesh_smooth_workspace_bytes(V, 0); with a ws_bytes between that and the
 * size prepare was given, no row beyond ws_bytes is read (such a vertex does not move).  A face index outside [0, V), a non-finite
 * vertex coordinate or a vertex outside the lattice is never used to address memory: the
 * kernels skip the element and set a device error word, which prepare reads and returns as
 * SDFR_EINVAL ("... outside [0, V)" / "... not finite" / "... outside the lattice").
 * Everything but that read is asynchronous on stream; nothing allocates.
 * ------------------------------------------------------------------------- */
size_t sdfr_mesh_smooth_workspace_bytes(uint32_t V, uint32_t F);
int sdfr_mesh_smooth_prepare(const float *verts, const int32_t *faces, uint32_t V, uint32_t F,
                             float ox, float oy, float oz, int unit_log2, int pin_boundary,
                             void *ws, size_t ws_bytes, int32_t *valence, uint8_t *boundary,
                             void *stream);
int sdfr_mesh_smooth_run(const float *verts, uint32_t V, const float *weights,
                         uint32_t n_passes, const void *ws, size_t ws_bytes, float *verts_out,
                         void *stream);

/* ---------------------------------------------------------------------------
 * Mesh rasteriser (added to ABI 15 without a version step: additive; csrc/raster.hip):
 * B views of one indexed mesh with the render's own pinhole camera, the nearest triangle
 * per pixel, deterministic.  Where the reference rasterises with pytorch3d
 * (sdf_model.py:754-782, sdf_utils.py:209-331).  Every floating-point step below is one
 * rounded fp32 operation (fadd / fsub / fmul / fdiv = round to nearest even, nothing
 * contracted), every integer step exact in int64, so a NumPy float32 / int64 transcription
 * (tests/raster_ref.py) gives the same bits.
 *
 * Vertex.  cam [B,3,4] is camera-to-world (rotation R = cam[:, :, :3], origin t =
 * cam[:, :, 3]).  d_m = fsub(v_m, t_m); the camera-frame point
 *   q_k = fadd(fadd(fmul(d_0, R[0][k]), fmul(d_1, R[1][k])), fmul(d_2, R[2][k]));
 * the depth z = -q_2; the screen position
 *   x = fadd(cx, fdiv(fmul(focal, q_0), z)),   y = fsub(cy, fdiv(fmul(focal, q_1), z)).
 * This inverts the render's ray generation: the pixel centre (i + 0.5, j + 0.5) with
 * cx = cy = res / 2 is the ray of pixel (column i, row j).
 * Fixed point, twelve subpixel bits: X = rint(fmul(x, 4096)), Y = rint(fmul(y, 4096))
 * (round half to even); rz = fdiv(1, z).  A vertex is unusable when z is not finite,
 * !(z > znear), or X or Y is not finite or has magnitude >= 2^30.
 *
 * Triangle (a, b, c), id = its row in faces.  Culled whole when an index is outside
 * [0, V), a vertex is unusable, or the doubled area
 *   A = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa)
 * is 0.  No back-face culling.
 *
 * Coverage of pixel (i, j), centre (Px, Py) = (4096 i + 2048, 4096 j + 2048):
 *   w1 = (Px - Xa)(Yc - Ya) - (Py - Ya)(Xc - Xa)
 *   w2 = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa)
 *   w0 = A - w1 - w2,
 * all three negated when A < 0; covered when all are >= 0 (edges inclusive: a pixel centre
 * on an edge two triangles share belongs to both, and the resolve decides).
 *
 * Depth and barycentrics.  l_i = fdiv(float(w_i), float(|A|)) (int64 -> fp32, nearest
 * even); iz = fadd(fadd(fmul(l0, rz_a), fmul(l1, rz_b)), fmul(l2, rz_c));
 * depth = fdiv(1, iz); the perspective-correct bary_i = fmul(fmul(l_i, rz_i), depth).
 * depth is the camera depth (the ray parameter of the render's unnormalised direction,
 * whose camera z is -1).  A depth that is not a positive finite number covers nothing.
 *
 * Resolve.  Each pixel keeps the minimum of the key (bits(depth) << 32) | id over the
 * triangles that cover it: the nearest one, the smallest id among equal depths.  The
 * minimum does not depend on the order in which triangles arrive, so the result is
 * reproducible bit for bit.
 *
 * Outputs (each may be NULL, one is required): face_idx [B,H,W] int32 (-1: uncovered),
 * depth [B,H,W], bary [B,H,W,3]; an uncovered pixel's depth and bary are 0.
 * Workspace, regions in order, each rounded up to 256 bytes: projected vertices
 * [B V] (X, Y, z, rz) 16 B | keys [B H W] 8 B | a counter (256 B) | the list of the
 * triangles whose clamped bounding box exceeds 64 pixels [B F] 8 B.  The size function
 * returns 0 for zero sizes, H or W above 16384, and B V, B F or B H W at or above 2^31.
 * SDFR_EINVAL before any launch for null arguments or required pointers, zero sizes,
 * every output null, znear negative or not finite, sizes the size function rejects, or a
 * workspace below its value.  Asynchronous on `stream`; allocates nothing; nothing is
 * read back.
 *
 * sdfr_mesh_interpolate: out[b, c, j, i] for the C channels of a per-vertex attribute
 * attr [V, C]: with (i0, i1, i2) the face face_idx[b, j, i] names,
 *   fadd(fadd(fmul(bary0, attr[i0, c]), fmul(bary1, attr[i1, c])), fmul(bary2, attr[i2, c]));
 * where face_idx is outside [0, F) (uncovered) or the face has an index outside [0, V):
 * background[b or 0, c, j, i] when a background is given ([background_batch, C, H, W],
 * background_batch 1 or B), else fill.  SDFR_EINVAL for null pointers, zero sizes, a
 * background_batch that is neither 1 nor B, or B C H W at or above 2^31.
 * ------------------------------------------------------------------------- */
typedef struct sdfr_raster_args {
    uint32_t B, H, W, V, F;           /* views, image rows, cols, vertices, triangles       */
    const float *vertices;            /* [V,3]                                              */
    const int32_t *faces;             /* [F,3]                                              */
    const float *cam;                 /* [B,3,4] camera-to-world                            */
    const float *focal;               /* [B] (device)                                       */
    float cx, cy, znear;
    int32_t *face_idx;                /* [B,H,W], optional                                  */
    float *depth;                     /* [B,H,W], optional                                  */
    float *bary;                      /* [B,H,W,3], optional                                */
    void *workspace; size_t workspace_bytes;
} sdfr_raster_args;
size_t sdfr_mesh_raster_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t V,
                                        uint32_t F);
int sdfr_mesh_raster(const sdfr_raster_args *a, void *stream);
int sdfr_mesh_interpolate(const float *attr, uint32_t V, uint32_t C, const int32_t *faces,
                          uint32_t F, const int32_t *face_idx, const float *bary, uint32_t B,
                          uint32_t H, uint32_t W, const float *background,
                          uint32_t background_batch, float fill, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFR_H_ */

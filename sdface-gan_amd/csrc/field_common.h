// field_common.h -- what the split-fp16 field kernels share (described in field_f16x3.hip):
// the network policies, the K permutations of the packed weights, the argument structs of
// the packing and field kernels, and fill_xfield_weights.  The kernels themselves are in
// field_pack.h (xprep_kernel), field_r.h (field_r_kernel, one wave per SIMD) and field_p.h
// (field_p_kernel, a wave pair per SIMD); a unit includes the headers of what it
// instantiates.
//
// Templates only.  A kernel is instantiated by the unit that launches it and by no other:
// the render's in field_f16x3.hip, the point queries' in field_query.hip and
// field_fc_query.hip, and field_grad.hip builds its gradient kernel on field_r.h's k-step
// loop (rstep) and packs with xprep_kernel (why: see NgpQueryNet below).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "f16x3.h"
#include "render_launch.h"
#include "render_ngp.h"

namespace sdfr {

constexpr uint32_t kXSliceF4 = 1024;             // 16 KB: [8 tiles][hi,lo][64 lanes] x 16 B
// ----------------------------------------------------------------------------
// network policies.  Weight matrices ("layers") in order: layer 0, the dense
// 256x256 layers, the views layer.  One packed slice per k-step of 16 input features
// (8 output tiles of 32 rows): layer 0 has 2 (ngp, 32 features) or 1 (siren, xyz)
// k-steps, the dense layers 16, the views layer 17 (256 + 16 SH / 3 direction inputs).
// ----------------------------------------------------------------------------
struct NgpNet {
    static constexpr bool kSiren = false;
    static constexpr bool kGrid = true;        // layer-0 inputs from the hash-grid encode kernel
    static constexpr bool kPosEnc = false;     // layer-0 / views inputs: positional encodings
    static constexpr bool kSinAct = true;      // FiLM sin activations (else ReLU)
    static constexpr int kL0 = 2;              // layer-0 k-steps of 16 K
    static constexpr int kViewSteps = 17;      // views-layer k-steps (256 hidden + 16 SH)
    static constexpr bool kFieldR = true;      // field_r_kernel (else field_p_kernel)
    static constexpr bool kQuery = false;      // field query at caller points (NgpQueryNet)
    // input_linear (LinearLayer, affine: sdf_model.py:37-39) feeds pts_linears.0's
    // linear with no nonlinearity between them (:1574-1577), so the two are ONE affine
    // map W1 (W0 x + b0) + b1 = (W1 W0) x + (W1 b0 + b1), composed once per weight
    // version in fp64 (compose_kernel): layer 0 is that 32 -> 256 map with
    // pts_linears.0's FiLM, and the 256 x 256 GEMM of pts_linears.0 per sample is gone.
    static constexpr bool kCompose = true;
    static constexpr int kLayers = 4;          // composed 0, pts_linears.1-2, views
    static constexpr int kFilmN = 4;           // FiLM: pts_linears.0-2, views
    static constexpr int kHidden = 2;          // dense layers after layer 0
    static constexpr uint32_t kSlices = 2 + 16 * 2 + 17;     // k-steps of 16 K per pass
    __host__ __device__ static constexpr uint32_t K(int l) {
        return l == 0 ? kFeatIn : (l == 3 ? kViewsIn : kW);
    }
    __host__ __device__ static constexpr int film_layer(int f) { return f; }
};
struct SirenNet {
    static constexpr bool kSiren = true;
    static constexpr bool kGrid = false;
    static constexpr bool kPosEnc = false;
    static constexpr bool kSinAct = true;
    static constexpr int kL0 = 1;
    static constexpr int kViewSteps = 17;
    static constexpr bool kFieldR = false;
    static constexpr bool kQuery = false;
    static constexpr bool kCompose = false;
    static constexpr bool kSlice2 = false;
    static constexpr int kLayers = 9;          // pts_linears.0-7, views
    static constexpr int kFilmN = 9;
    static constexpr int kHidden = 7;
    static constexpr uint32_t kSlices = 2 + 16 * 7 + 18;     // field_p_kernel's half-slices
    __host__ __device__ static constexpr uint32_t K(int l) {
        return l == 0 ? 3u : (l == 8 ? kW + 3 : kW);
    }
    __host__ __device__ static constexpr int film_layer(int f) { return f; }
};
// FCGenerator (rendering.fc == 1, sdf_model.py:1599-1670): positional encodings of the
// normalised point (3 x 10 frequencies x sin, cos = 60) -> x_in (+ style_in(styles), a
// per-face bias) -> ReLU -> 7 x (256 -> 256, ReLU) -> sigma | [h7, posenc(view) (24)] ->
// views (no activation: the colour features) -> rgb.  Every layer is affine then ReLU,
// run as ReLU(fma(1/su, z, b)) on the row-scaled GEMM output z (1/su exact), i.e. the
// FiLM slot with gamma'' = 1/su and beta'' = the bias.
struct FcNet {
    static constexpr bool kSiren = false;
    static constexpr bool kGrid = false;
    static constexpr bool kPosEnc = true;
    static constexpr bool kSinAct = false;
    static constexpr int kL0 = 4;              // 60 encodings (+ 4 zero pad)
    static constexpr int kViewSteps = 18;      // 256 hidden + 24 view encodings (+ 8 pad)
    static constexpr bool kFieldR = true;
    static constexpr bool kQuery = false;
    static constexpr bool kCompose = false;
    static constexpr int kLayers = 9;          // x_in, pts_linears.0-6, views
    static constexpr int kFilmN = 9;           // (1/su, bias) per layer; layer 0 per face
    static constexpr int kHidden = 7;
    static constexpr uint32_t kSlices = 4 + 16 * 7 + 18;
    static constexpr uint32_t kPosIn = 60, kPosViews = 24;
    __host__ __device__ static constexpr uint32_t K(int l) {
        return l == 0 ? kPosIn : (l == 8 ? kW + kPosViews : kW);
    }
    __host__ __device__ static constexpr int film_layer(int f) { return f; }
};
// NgpNet in query mode (sdfr_query_ngp_forward, csrc/field_query.hip): field_r_kernel
// evaluates the field at the caller's points -- H = 1, W = R direction groups, N points
// per group; the group's unit direction is read from memory (XFieldArgs::g.cam holds
// dirs [B,R,3]) instead of built from a camera, compositing is compiled out, and every
// sample stores its SDF ([B,R,N]) and sigmoid(rgb) ([B,R,N,3]).  Same packed weights,
// FiLM vectors and per-sample arithmetic as the render.  Instantiated in its own
// translation unit only: co-compiled instantiations of one template perturb each
// other's register allocation, and the render kernels' code must not move.
struct NgpQueryNet : NgpNet {
    static constexpr bool kQuery = true;
};
// (SirenNet's query policy, SirenQueryNet, puts field_p_kernel into the same mode -- the
// points [B,R,N,3] arrive in XFieldArgs::enc, which the SIREN render leaves unused; it is
// declared where it is instantiated, csrc/field_query.hip.  FcNet's, FcQueryNet, is
// field_r_kernel's as NgpQueryNet is, with the point read from XFieldArgs::enc as well; it
// is declared and instantiated in csrc/field_fc_query.hip.)

// field_p_kernel's packing (SirenNet): slices = 2 per k-step of 32 input features
// (8 output tiles of 16 rows each); layer 0 one k-step, dense layers 8, views 9.
template <class Net>
__host__ __device__ constexpr uint32_t xslice_base(int l) {
    return l == 0 ? 0u : (l == Net::kLayers - 1 ? 2u + 16u * Net::kHidden : 2u + 16u * (l - 1));
}

// K index of element j of lane group g in field_p_kernel's k-step q of layer l
// (-1 = zero pad).
template <class Net>
__device__ __forceinline__ int xperm_k(int l, uint32_t q, uint32_t g, uint32_t j) {
    if (l == 0) {
        if constexpr (Net::kSiren) return (g == 0 && j < 3) ? (int)j : -1;   // xyz
        return (int)(8 * g + j);                                           // 32 features
    }
    if (l == Net::kLayers - 1 && q == 8) {
        if constexpr (Net::kSiren) return (g == 0 && j < 3) ? (int)(kW + j) : -1;   // viewdir
        return g < 2 ? (int)(kW + 8 * g + j) : -1;                                // SH 0-15
    }
    return (int)(16 * (2 * q + (j >> 2)) + 4 * g + (j & 3));
}

constexpr int kRWaves = 4;
constexpr int kRThreads = kRWaves * 64;
constexpr uint32_t kRTiles = 4;          // 16-ray tiles per workgroup (one per wave)
constexpr uint32_t kRSamples = 2;        // samples of a ray per pass
constexpr uint32_t kRSliceF4 = 1024;     // 16 KB: one k-step's [8 tiles][hi, lo][64 lanes]

typedef float f16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f16v mfma32(f4 a, f4 b, f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), as_h8(b), c, 0, 0, 0);
}

template <class Net>
struct RNet {
    static constexpr int kL0 = Net::kL0;                           // layer-0 k-steps (K 3 / 32 / 60)
    static constexpr int kSteps = kL0 + 16 * Net::kHidden + Net::kViewSteps;   // (slices) per pass
    static constexpr int kViews = kL0 + 16 * Net::kHidden;         // first views k-step
    static_assert(!Net::kFieldR || kSteps == (int)Net::kSlices, "one packed slice per k-step");
};

template <class Net>
__host__ __device__ constexpr uint32_t rslice_base(int l) {
    return l == 0 ? 0u
                  : (uint32_t)RNet<Net>::kL0 + 16u * (l == Net::kLayers - 1 ? Net::kHidden : l - 1);
}

// K index (within layer l's input) of element j of lane half h in the layer's k-step s
// (-1 = zero pad)
template <class Net>
__device__ __forceinline__ int rperm_k(int l, uint32_t s, uint32_t h, uint32_t j) {
    const uint32_t e = 8 * h + j;
    if (l == 0) {
        if constexpr (Net::kSiren) return e < 3 ? (int)e : -1;   // xyz
        if constexpr (Net::kPosEnc) return 16 * s + e < Net::kPosIn ? (int)(16 * s + e) : -1;
        return (int)(16 * s + e);                               // 32 grid features
    }
    if (l == Net::kLayers - 1 && s >= 16) {
        if constexpr (Net::kSiren) return e < 3 ? (int)(kW + e) : -1;   // viewdir
        if constexpr (Net::kPosEnc)                                     // view encodings
            return 16 * (s - 16) + e < Net::kPosViews ? (int)(kW + 16 * (s - 16) + e) : -1;
        return (int)(kW + e);                                           // SH 0-15
    }
    return (int)(32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3));
}

// ----------------------------------------------------------------------------
// prep 2 (xprep_kernel, field_pack.h): FiLM vectors (gamma / su) + split-fp16 weight
// fragments
// ----------------------------------------------------------------------------
struct XPrepArgs {
    const float *styles;           // [B,256]
    const float *gw[kMaxLayers], *gb[kMaxLayers], *bw[kMaxLayers], *bb[kMaxLayers];
    const float *w[kMaxLayers];
    const float *lb[kMaxLayers];   // layer biases (unscaled)
    const float *su;               // [layers][256]
    float *film;                   // [B][films][2][256]
    f4 *packed;                    // [slices][8][2][64] fp16x8
    uint32_t B;
};

// ----------------------------------------------------------------------------
// field kernels (field_r.h, field_p.h)
// ----------------------------------------------------------------------------
struct XFieldArgs {
    GeomArgs g;                    // (query mode: H = 1, W = R, cam = dirs [B,R,3])
    const float *enc;              // ngp: [L=16][S_total][2]; siren: unused
    const float2 *zd;              // ngp: [S_total] (z, segment length) from the encode kernel
    const f4 *packed;              // [slices][1024]
    const float *film;             // [B][films][2][256], gamma pre-divided by su
    const float *su;               // [layers][256]
    const float *bias_s;           // [layers][256]
    const float *sigma_w, *sigma_b, *rgb_w, *rgb_b, *sigmoid_beta;
    const float *sigma_noise;      // [B,H,W,N] or null (no_sdf only)
    int force_background, with_sdf;
    float *rgb, *features, *sdf, *xyz, *mask;
    _Float16 *feat_split;          // or the features x feat_mod in split-NHWC (ABI 12)
    const float *feat_mod;         // [B][256]
    uint32_t nseg;                 // sample segments per ray (1: whole rays, no merge)
    float *part;                   // nseg > 1: [nseg][kPartQ][rays] segment partials
};

// Small batches (eval.py renders one face per call) fill a fraction of the chip
// with one workgroup per 4 tiles: the 24 samples of a ray are then split into
// nseg segments marched by different workgroups, each compositing its samples
// front to back from T = 1, and field_merge_kernel chains the segments
// (acc = acc_1 + T_1 acc_2 + T_1 T_2 acc_3 ..., T = prod T_k), which is the
// same sum with the transmittance product re-associated (fp32-rounding-level
// differences; tests/test_gpu_render.py compares split and unsplit renders).
// Partials per (segment, ray): 256 features, rgb[3], xyz[3], T, w_last.
constexpr uint32_t kPartQ = kW + 8;

template <int B, int E, class F>
__device__ __forceinline__ void sfor(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        sfor<B + 1, E>(f);
    }
}

// The weight part of a field launch's arguments: the region `xws` in xprep_kernel's layout
// (packed [slices][1024] f4 | su [L][256] | bias_s [L][256]), the FiLM vectors and the heads.
template <class Net>
void fill_xfield_weights(XFieldArgs &f, const NetPtrs &P, const char *xws, const float *film) {
    f.packed = reinterpret_cast<const f4 *>(xws);
    f.su = reinterpret_cast<const float *>(xws + (size_t)Net::kSlices * kXSliceF4 * sizeof(f4));
    f.bias_s = f.su + Net::kLayers * kW;
    f.film = film;
    f.sigma_w = P.sigma_w;
    f.sigma_b = P.sigma_b;
    f.rgb_w = P.rgb_w;
    f.rgb_b = P.rgb_b;
    f.sigmoid_beta = P.sigmoid_beta;
}

}  // namespace sdfr

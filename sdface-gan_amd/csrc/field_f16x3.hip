// field_f16x3.hip -- the fused renderer's field stage on split-fp16 MFMA, for
// both SDFace networks:
//
//   NgpNet    NGPSIRENGenerator (sdf_model.py:1534-1592): hash-grid features (32)
//             -> input_linear -> 3 FiLM layers -> sigma | [h3, SH(16)] -> views
//             FiLM -> rgb.  Inputs come from the hash-grid encode kernel.
//   SirenNet  SirenGenerator (sdf_model.py:101-139): normalised points (3) -> 8
//             FiLM layers -> sigma | [h7, viewdir(3)] -> views FiLM -> rgb.
//             Points are formed in-kernel from the ray (bit-exact chain).
//
// followed by SDF->density and front-to-back alpha compositing
// (volume_integration, :236-301).  Every fp32 GEMM tile runs as three fp16 MFMAs
// (v_mfma_f32_32x32x16_f16 for ngp, v_mfma_f32_16x16x32_f16 for siren) on a hi/lo
// fp16 split of both operands:
//
//     W.x = W_hi.x_hi + W_hi.x_lo + W_lo.x_hi   (+ W_lo.x_lo, dropped: 2^-22 rel.)
//
// accumulated in fp32 by the matrix core: 5.3x the fp32 MFMA rate.  Accuracy
// (scripts/probe_split_f16.hip, measured on MI355X): a 256-deep dot product is as
// accurate as the fp32 fma chain PROVIDED the fp16 lo parts do not go subnormal --
// so every weight row is scaled by a power of two su (max |w| su in [0.5,1),
// xscale_kernel) and every sample's features by a power of two before the split.
// Power-of-two scaling commutes with rounding, so it is undone exactly: the FiLM
// gamma is divided by su (gamma' x_scaled == gamma x, bit for bit), the layer bias
// folds into the FiLM beta, and the feature scale is taken out in layer 0's FiLM.
//
// Work unit (field_r_kernel, field_r.h): a workgroup of 4 waves, one per SIMD (512
// VGPRs), over 4 tiles of 16 rays; each wave computes ALL 256 output rows of every
// layer for 32 samples (16 rays x 2 consecutive samples), so a layer's accumulators,
// activated and split in place, are the next layer's B fragments (no LDS hand-off).
// The weight stream (0.8 MB per pass) is shared by the 4 waves through a 4-slot
// LDS-DMA ring of 16 KB slices (one per k-step of 16 K), with the packed weights' K
// permuted to match the accumulator layout (xprep_kernel).  The SIREN net runs on
// field_p_kernel (two waves per SIMD splitting each layer's rows, its own packing:
// 16 KB half-slices per k-step of 32 K), which is 6 % faster on its nine FiLM layers
// -- the one-wave kernel's 32x32 MFMAs hold a lower clock there (1.64 GHz, counters).
//
// The kernel templates are in field_pack.h, field_p.h and field_r.h (what they share in
// field_common.h).  This unit holds the render's instantiations of them with their
// launches (launch_xprep, launch_xfield), the non-template kernels (xscale_kernel,
// compose_kernel, field_merge_kernel) and the sample-segment rule (field_nseg).  The entry
// points that call them are in render_api.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "field_common.h"
#include "field_pack.h"
#include "field_p.h"
#include "field_r.h"
#include "render_launch.h"

namespace sdfr {

// ----------------------------------------------------------------------------
// prep 1: per-row power-of-two scales and scaled biases (one wave per row)
// ----------------------------------------------------------------------------
struct XScaleArgs {
    const float *w[kMaxLayers];
    const float *b[kMaxLayers];
    uint32_t K[kMaxLayers];
    float *su;       // [layers][256]
    float *bias_s;   // [layers][256]
    int raw_bias0;   // layer 0's bias stays unscaled (ngp: added after the GEMM)
};

__global__ void __launch_bounds__(256) xscale_kernel(const XScaleArgs a) {
    const uint32_t layer = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.y * 4 + (threadIdx.x >> 6);
    const uint32_t K = a.K[layer];
    const float *wr = a.w[layer] + (size_t)row * K;
    float m = 0.0f;                        // max is order-independent: exact
    for (uint32_t k = lane; k < K; k += 64) m = fmaxf(m, fabsf(wr[k]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane != 0) return;
    float su = 1.0f;
    if (m > 0.0f && m < 3.0e38f) {
        int ex;
        (void)frexpf(m, &ex);              // m = f 2^ex, f in [0.5, 1)
        ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
        su = ldexpf(1.0f, -ex);
    }
    a.su[layer * kW + row] = su;
    a.bias_s[layer * kW + row] =
        (layer == 0 && a.raw_bias0) ? a.b[0][row] : __fmul_rn(a.b[layer][row], su);
}

// prep 0 (ngp): layer 0 = pts_linears.0 o input_linear, one row per block, fp64 sums
// rounded once to fp32: wc = W1 W0 [256][32], bc = W1 b0 + b1 [256]
__global__ void __launch_bounds__(64) compose_kernel(const float *w0, const float *b0,
                                                     const float *w1, const float *b1,
                                                     float *wc, float *bc) {
    const uint32_t i = blockIdx.x, j = threadIdx.x;
    if (j > kFeatIn) return;
    const float *r1 = w1 + (size_t)i * kW;
    double acc = j < kFeatIn ? 0.0 : (double)b1[i];
    for (uint32_t k = 0; k < kW; ++k)
        acc = fma((double)r1[k], j < kFeatIn ? (double)w0[(size_t)k * kFeatIn + j] : (double)b0[k], acc);
    if (j < kFeatIn) wc[(size_t)i * kFeatIn + j] = (float)acc;
    else bc[i] = (float)acc;
}

// Chains the nseg segment partials of every ray (see kPartQ): one thread per
// (ray, quantity), quantities on grid.y.
__global__ void __launch_bounds__(256) field_merge_kernel(const XFieldArgs a) {
    const GeomArgs &G = a.g;
    const uint32_t rid = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
    const size_t R = (size_t)G.total_tiles * kTileRays;
    if (rid >= R) return;
    const uint32_t tile = rid / kTileRays, b = tile / G.tiles_per_face;
    const uint32_t ray_local = (tile % G.tiles_per_face) * kTileRays + rid % kTileRays;
    const size_t HW = (size_t)G.H * G.W;
    if (ray_local >= HW) return;
    float *dst;
    float fsplit = 0.0f;                                 // (any non-null marker)
    if (q < kW) dst = a.features ? a.features + ((size_t)b * kW + q) * HW + ray_local
                                 : (a.feat_split ? &fsplit : nullptr);
    else if (q < kW + 3) dst = a.rgb + ((size_t)b * 3 + (q - kW)) * HW + ray_local;
    else if (q < kW + 6) dst = a.xyz ? a.xyz + ((size_t)b * 3 + (q - kW - 3)) * HW + ray_local
                                     : nullptr;
    else if (q == kW + 7) dst = a.mask ? a.mask + (size_t)b * HW + ray_local : nullptr;
    else dst = nullptr;                                  // T itself is not an output
    if (!dst) return;
    const float *pp = a.part + rid;
    const size_t segq = (size_t)kPartQ * R;
    float acc = pp[(size_t)q * R], Tp = pp[(size_t)(kW + 6) * R];
    for (uint32_t k = 1; k < a.nseg; ++k) {
        const float v = pp[k * segq + (size_t)q * R];
        acc = q == kW + 7 ? __fmul_rn(Tp, v) : __fmaf_rn(Tp, v, acc);   // w_last: last segment's
        Tp = __fmul_rn(Tp, pp[k * segq + (size_t)(kW + 6) * R]);
    }
    if (q >= kW && q < kW + 3) acc = __fadd_rn(-1.0f, __fmul_rn(2.0f, acc));
    if (dst == &fsplit) {                                // split-NHWC, times the modulation
        float v = __fmul_rn(acc, a.feat_mod[(size_t)b * kW + q]);
        asm volatile("" : "+v"(v));      // (no v_fma_mix fold of the product: see above)
        const _Float16 hv = (_Float16)v, lv = (_Float16)(v - (float)hv);
        const size_t o = 2 * (((size_t)b * HW + ray_local) * kW + (q & ~7u)) + (q & 7u);
        a.feat_split[o] = hv;
        a.feat_split[o + 8] = lv;
        return;
    }
    *dst = acc;
}

// ----------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------
// Sample segments per ray: enough workgroups for every CU (>= 256), at most max_seg
// (the call's max_field_segments, 0 = kFieldSplitMax), at least one pass (4 samples)
// in every segment, and never with force_background (its last weight needs the
// whole ray's sum).
uint32_t field_nseg(uint32_t B, uint32_t tiles_per_face, uint32_t N, int force_background,
                    uint32_t max_seg) {
    if (max_seg == 0 || max_seg > kFieldSplitMax) max_seg = kFieldSplitMax;
    const uint32_t wgs = B * ((tiles_per_face + kRTiles - 1) / kRTiles);
    const uint32_t npass = (N + kRSamples - 1) / kRSamples;
    uint32_t nseg = 1;
    while (!force_background && wgs * nseg < 256 && 2 * nseg <= max_seg) {
        const uint32_t c = 2 * nseg, pps = (npass + c - 1) / c;
        if ((c - 1) * pps >= npass) break;            // no empty last segment
        nseg = c;
    }
    return nseg;
}

size_t field_part_bytes(uint32_t B, uint32_t tiles_per_face, uint32_t N) {
    const uint32_t nseg = field_nseg(B, tiles_per_face, N, 0, kFieldSplitMax);
    return nseg > 1 ? (size_t)nseg * kPartQ * B * tiles_per_face * kTileRays * sizeof(float) : 0;
}

static_assert(NgpNet::kFilmN == kFilm && SirenNet::kFilmN == kSirenFilm &&
                  FcNet::kFilmN == kFcFilm && SirenNet::kLayers <= kMaxLayers,
              "the entry points size the film region with these");

template <class Net>
static size_t xws_bytes() {
    return (size_t)Net::kSlices * kXSliceF4 * sizeof(f4) + 2 * Net::kLayers * kW * sizeof(float) +
           (Net::kCompose ? (size_t)(kFeatIn + 1) * kW * sizeof(float) : 0);
}

// the composed ngp layer 0 inside the region: W [256][32] | b [256]
template <class Net>
static float *xws_composed(char *xws) {
    return reinterpret_cast<float *>(xws + (size_t)Net::kSlices * kXSliceF4 * sizeof(f4)) +
           2 * Net::kLayers * kW;
}

// workspace region of this path: packed [slices][1024] f4 | su [L][256] | bias_s [L][256]
// (| composed layer 0, ngp)
size_t f16x3_ws_bytes(int net) {
    return net == kNetFc ? xws_bytes<FcNet>()
                         : (net == kNetNgp ? xws_bytes<NgpNet>() : xws_bytes<SirenNet>());
}

int launch_xscale(const float *const *w, const float *const *b, const uint32_t *K, int layers,
                  float *su, float *bias_s, hipStream_t st) {
    XScaleArgs sa{};
    for (int l = 0; l < layers; ++l) {
        sa.w[l] = w[l];
        sa.b[l] = b[l];
        sa.K[l] = K[l];
    }
    sa.su = su;
    sa.bias_s = bias_s;
    sa.raw_bias0 = 0;
    hipLaunchKernelGGL(xscale_kernel, dim3(layers, kW / 4), dim3(256), 0, st, sa);
    return check_launch("render: xscale");
}

// Per call: the per-face FiLM blocks of xprep_kernel (styles / film; film null: none) and,
// with `pack`, the row scales, scaled biases and packed MFMA A-fragments (xscale_kernel +
// the packing blocks of xprep_kernel) into `xws`.  Without `pack` xws holds them already
// (weights packed beforehand: sdfr_render_*_pack).
template <class Net>
static int launch_xpack(const NetPtrs &P, uint32_t B, const float *styles, char *xws, float *film,
                        bool pack, hipStream_t st) {
    f4 *packed = reinterpret_cast<f4 *>(xws);
    float *su = reinterpret_cast<float *>(xws + (size_t)Net::kSlices * kXSliceF4 * sizeof(f4));
    float *bias_s = su + Net::kLayers * kW;
    NetPtrs Q = P;
    if constexpr (Net::kCompose) {
        float *wc = xws_composed<Net>(xws);
        Q.w[0] = wc;
        Q.b[0] = wc + kFeatIn * kW;
        if (pack) {
            hipLaunchKernelGGL(compose_kernel, dim3(kW), dim3(64), 0, st, P.in_w, P.in_b, P.p0_w,
                               P.p0_b, wc, wc + kFeatIn * kW);
            int rc = check_launch("render: compose layer 0");
            if (rc) return rc;
        }
    }
    if (pack) {
        uint32_t K[kMaxLayers];
        for (int l = 0; l < Net::kLayers; ++l) K[l] = Net::K(l);
        int rc = launch_xscale(Q.w, Q.b, K, Net::kLayers, su, bias_s, st);
        if (rc) return rc;
    }
    XPrepArgs p;
    p.styles = styles;
    for (int f = 0; f < Net::kFilmN; ++f) {
        p.gw[f] = P.gw[f];
        p.gb[f] = P.gb[f];
        p.bw[f] = P.bw[f];
        p.bb[f] = P.bb[f];
    }
    for (int l = 0; l < Net::kLayers; ++l) {
        p.w[l] = Q.w[l];
        p.lb[l] = Q.b[l];
    }
    p.su = su;
    p.film = film;
    p.packed = packed;
    p.B = film ? B : 0;
    // blocks [0, B films x 2 x 256 / 4): FiLM rows; then (pack) the fragment packing
    const uint32_t nfilm = p.B * Net::kFilmN * 2 * kW / 4;
    const uint32_t blocks = nfilm + (pack ? (Net::kSlices * 512 + 255) / 256 : 0);
    if (blocks == 0) return SDFR_OK;
    hipLaunchKernelGGL(xprep_kernel<Net>, dim3(blocks), dim3(256), 0, st, p);
    return check_launch("render: xprep");
}

template <class Net>
static int launch_xfield(const NetPtrs &P, const sdfr_ngp_render_args *a, const GeomArgs &g,
                         const float *enc, const char *xws, const float *film, hipStream_t st,
                         float *part, const float2 *zd) {
    XFieldArgs f;
    f.g = g;
    f.enc = enc;
    f.zd = zd;
    fill_xfield_weights<Net>(f, P, xws, film);
    f.sigma_noise = a->sigma_noise;
    f.force_background = a->force_background;
    f.with_sdf = a->with_sdf;
    f.rgb = a->rgb;
    f.features = a->features;
    f.feat_split = reinterpret_cast<_Float16 *>(a->features_split);
    f.feat_mod = a->features_mod;
    f.sdf = a->sdf;
    f.xyz = a->xyz;
    f.mask = a->mask;
    f.part = part;
    if (f.feat_split && (!f.feat_mod || f.features || !Net::kFieldR))
        return fail(SDFR_EUNSUPPORTED, "render: features_split needs features_mod, no NCHW "
                                       "features, and the ngp / FC field kernel");
    // field_r_kernel for ngp; the SIREN net (nine FiLM layers, no encode stage, no
    // sample-segment split) keeps field_p_kernel, 6 % faster on it (7.76 vs 8.25 ms per
    // 32 faces, interleaved A/B on one box; field_r_kernel is 3.5 % faster on ngp)
    if constexpr (Net::kFieldR) {
        f.nseg = part ? field_nseg(g.B, g.tiles_per_face, g.N, a->force_background,
                                   a->max_field_segments) : 1;
        const uint32_t blocks = g.B * ((g.tiles_per_face + kRTiles - 1) / kRTiles) * f.nseg;
        hipLaunchKernelGGL((field_r_kernel<Net>), dim3(blocks), dim3(kRThreads), 0, st, f);
    } else {
        if (part) return fail(SDFR_EUNSUPPORTED, "render: field_p_kernel has no segment split");
        f.nseg = 1;
        const uint32_t blocks = g.B * ((g.tiles_per_face + kPTiles - 1) / kPTiles);
        hipLaunchKernelGGL((field_p_kernel<Net>), dim3(blocks), dim3(kPThreads), 0, st, f);
    }
    int rc = check_launch("render: field (f16x3)");
    if (rc || f.nseg == 1) return rc;
    const uint32_t rays = g.total_tiles * kTileRays;
    hipLaunchKernelGGL(field_merge_kernel, dim3((rays + 255) / 256, kPartQ), dim3(256), 0, st, f);
    return check_launch("render: field segment merge");
}

int launch_xprep(int net, const NetPtrs &P, uint32_t B, const float *styles, char *xws,
                 float *film, bool pack, hipStream_t st) {
    if (net == kNetNgp) return launch_xpack<NgpNet>(P, B, styles, xws, film, pack, st);
    if (net == kNetFc) return launch_xpack<FcNet>(P, B, styles, xws, film, pack, st);
    return launch_xpack<SirenNet>(P, B, styles, xws, film, pack, st);
}

int launch_xfield(int net, const NetPtrs &P, const sdfr_ngp_render_args *a, const GeomArgs &g,
                  const float *enc, const char *xws, const float *film, hipStream_t st,
                  float *part, const float2 *zd) {
    if (net == kNetNgp) return launch_xfield<NgpNet>(P, a, g, enc, xws, film, st, part, zd);
    if (net == kNetFc) return launch_xfield<FcNet>(P, a, g, enc, xws, film, st, part, zd);
    return launch_xfield<SirenNet>(P, a, g, enc, xws, film, st, part, zd);
}

}  // namespace sdfr

// conv_f16x3.hip -- the StyleGAN2 decoder's 3x3 convolutions on split-fp16 MFMA.
//
// Replaces the two convolution forms of ModulatedConv2d on the fused decoder
// path (sdf_model.py:676-699, applied as conv(x * s, w) * demod -- the batched
// form of the reference's per-face modulated weights, see generator.py):
//   regular     out[b,y,x,o]   = sum_{i,ky,kx} x[b,y+ky-1,x+kx-1,i] w[o,i,ky,kx]   (pad 1)
//   transposed  out[b,2a+ky,2c+kx,o] += x[b,a,c,i] w[o,i,ky,kx]   (conv_transpose2d,
//               stride 2, output (2H+1) x (2W+1), before the upsampling blur)
// as implicit GEMMs over NHWC activations: M = output channels (A = weights),
// N = output pixels (B = activations), K = input channels x taps.  Every fp32
// tile product is W_hi.x_hi + W_hi.x_lo + W_lo.x_hi on v_mfma_f32_16x16x32_f16
// with fp32 accumulation (the field kernel's scheme):
// 5.3x the fp32 MFMA rate at fp32-level accuracy.  Weights are row-scaled by a
// power of two su[o] so their fp16 lo parts stay normal; the caller folds 1/su
// into the demodulation (exact).  A transposed conv is four implicit GEMMs, one
// per output parity class (oy & 1, ox & 1), each over its own tap subset.
//
// This unit: the weight packing kernels, the launch of a plan's steps (conv_plan.h
// decides them; the kernels are templates in conv_x.h, conv_h.h and conv_t.h) and the
// C entry points.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>

#include "conv_h.h"
#include "conv_plan.h"
#include "conv_t.h"
#include "conv_x.h"
#include "sdfr_common.h"

namespace sdfr {
namespace {

// ----------------------------------------------------------------------------
// weight packing: w [Cout][Cin][3][3] * scale -> su [Cout], fragments
// [tap 9][Cin/32][Cout/128][8 m-tiles][hi, lo][64 lanes] fp16x8, lane (m, g)
// holding w[o = 16 mt + m][i = 32 c + 8 g + j][tap], j = 0..7
// ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv_scale_kernel(const float *__restrict__ w, float scale,
                                                         uint32_t Cin, float *__restrict__ su) {
    const uint32_t o = blockIdx.x;
    float m = 0.0f;
    for (uint32_t k = threadIdx.x; k < Cin * 9; k += 256)
        m = fmaxf(m, fabsf(__fmul_rn(w[(size_t)o * Cin * 9 + k], scale)));
    __shared__ float red[256];
    red[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float v = 1.0f;
        const float mx = red[0];
        if (mx > 0.0f && mx < 3.0e38f) {
            int ex;
            (void)frexpf(mx, &ex);
            ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
            v = ldexpf(1.0f, -ex);
        }
        su[o] = v;
    }
}

__global__ void __launch_bounds__(256) conv_pack_kernel(const float *__restrict__ w, float scale,
                                                        uint32_t Cin, uint32_t Cout,
                                                        const float *__restrict__ su,
                                                        f4 *__restrict__ packed) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;        // one (tap, c, cb, mt, lane)
    const uint32_t nC = Cin / 32, nB = Cout / kCT;
    const uint32_t total = 9 * nC * nB * 8 * 64;
    if (e >= total) return;
    const uint32_t lane = e & 63, mt = (e >> 6) & 7;
    uint32_t r = e >> 9;
    const uint32_t cb = r % nB;
    r /= nB;
    const uint32_t c = r % nC, tap = r / nC;
    const uint32_t o = cb * kCT + mt * 16 + (lane & 15), g = lane >> 4;
    const float s = su[o];
    h8 H, L;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t i = c * 32 + 8 * g + j;
        const float v = __fmul_rn(__fmul_rn(w[((size_t)o * Cin + i) * 9 + tap], scale), s);
        H[j] = (_Float16)v;
        L[j] = (_Float16)__fsub_rn(v, (float)H[j]);
    }
    f4 *dst = packed + ((size_t)(e >> 6) * 2) * 64 + lane;   // [.. mt][hi,lo][lane]
    dst[0] = __builtin_bit_cast(f4, H);
    dst[64] = __builtin_bit_cast(f4, L);
}

// The conv_t mode (sdfr_set_conv_t_mode; plan_conv describes the values): SDFR_CONV_T read
// once when the library loads.
int conv_t_env_mode() {
    const char *e = getenv("SDFR_CONV_T");
    return e ? atoi(e) : 1;
}
int g_conv_t_mode = conv_t_env_mode();

void launch_step(const ConvStep &s, const ConvArgs &a, hipStream_t st) {
    const dim3 g(s.gx, s.gy), b(s.block);
    switch (s.kernel) {
    case kKConvX: hipLaunchKernelGGL(conv_x_kernel<false>, g, b, 0, st, a); break;
    case kKConvXAct: hipLaunchKernelGGL(conv_x_kernel<true>, g, b, 0, st, a); break;
    case kKSplitK: hipLaunchKernelGGL(conv_splitk_kernel<false>, g, b, 0, st, a); break;
    case kKSplitKAct: hipLaunchKernelGGL(conv_splitk_kernel<true>, g, b, 0, st, a); break;
    case kKConvH: hipLaunchKernelGGL(conv_h_kernel<false>, g, b, 0, st, a); break;
    case kKConvHSplit: hipLaunchKernelGGL(conv_h_kernel<true>, g, b, 0, st, a); break;
    case kKConvHFinish: hipLaunchKernelGGL(conv_h_finish_kernel, g, b, 0, st, a); break;
    case kKConvT: hipLaunchKernelGGL(conv_t_kernel<false>, g, b, 0, st, a); break;
    case kKConvTFuse: hipLaunchKernelGGL(conv_t_kernel<true>, g, b, 0, st, a); break;
    case kKConvTFinish: hipLaunchKernelGGL(conv_t_finish_kernel, g, b, 0, st, a); break;
    case kKBorderRows: hipLaunchKernelGGL(conv_t_border_kernel<true>, g, b, 0, st, a); break;
    case kKBorderCols: hipLaunchKernelGGL(conv_t_border_kernel<false>, g, b, 0, st, a); break;
    }
}

// Plans the convolution (a: out, e and fir already set by the entry point), copies the
// plan into the kernel arguments and launches its steps.
int conv_run(ConvArgs &a, const ConvShape &s, const void *x_split, const void *packed, void *ws,
             hipStream_t st, const char *what) {
    if (!x_split || !packed) return fail(SDFR_EINVAL, std::string(what) + ": null pointer");
    const ConvPlan p = plan_conv(s, g_conv_t_mode);
    if (p.rc) return fail(p.rc, std::string(what) + ": " + p.msg);
    a.xs = reinterpret_cast<const _Float16 *>(x_split);
    a.wpk = reinterpret_cast<const f4 *>(packed);
    a.B = s.B;
    a.Hin = s.H;
    a.Win = s.W;
    a.Cin = s.Cin;
    a.Cout = s.Cout;
    a.Hf = p.Hf;
    a.Wf = p.Wf;
    a.sy = p.sy;
    a.ncls = p.ncls;
    for (uint32_t i = 0; i < 4; ++i) a.cls[i] = p.cls[i];
    for (int t = 0; t < 9; ++t) {
        a.dy[t] = p.dy[t];
        a.dx[t] = p.dx[t];
        a.tap[t] = p.tap[t];
    }
    a.grid = p.grid;
    a.ksplit = p.ksplit;
    a.partial = p.ksplit > 1 ? reinterpret_cast<f4 *>(ws) : nullptr;
    a.tiles_t = p.tiles_t;
    a.ksplit_t = p.ksplit_t;
    a.ptl = p.ksplit_t > 1 ? reinterpret_cast<float *>(ws) : nullptr;
    for (uint32_t i = 0; i < p.nsteps; ++i) {
        launch_step(p.steps[i], a, st);
        const int rc = check_launch(what);
        if (rc) return rc;
    }
    return SDFR_OK;
}

// the workspace from which the shape's path takes its split (0: none, or a refused shape)
size_t plan_ws_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t Cout, bool transposed, int epi) {
    // (the size does not depend on Cin: the smallest stands in)
    const ConvPlan p = plan_conv(ConvShape{B, H, W, 32, Cout, transposed, epi, false, 0}, g_conv_t_mode);
    return p.rc ? 0 : p.ws_bytes;
}

void set_act_epilogue(ActEpi &e, const float *demod, const float *noise, const float *noise_weight,
                      const float *bias, float slope, float scale, const float *s_next,
                      void *y_split) {
    e.demod = demod;
    e.noise = noise;
    e.noise_weight = noise_weight;
    e.bias = bias;
    e.slope = slope;
    e.scale = scale;
    e.s_next = s_next;
    e.ys = reinterpret_cast<_Float16 *>(y_split);
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" {

size_t sdfr_conv_pack_bytes(uint32_t Cout, uint32_t Cin) {
    return (size_t)9 * Cin * Cout * 2 * sizeof(_Float16) + (size_t)Cout * sizeof(float);
}

int sdfr_conv_pack_weights(const float *w, float scale, uint32_t Cout, uint32_t Cin,
                           void *packed, float *su, void *stream) {
    if (!w || !packed || !su) return fail(SDFR_EINVAL, "conv_pack_weights: null pointer");
    if (Cout == 0 || Cout % kCT || Cin == 0 || Cin % 32)
        return fail(SDFR_EINVAL, "conv_pack_weights: Cout % 128 and Cin % 32 must be 0");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv_scale_kernel, dim3(Cout), dim3(256), 0, st, w, scale, Cin, su);
    int rc = check_launch("conv_pack_weights: scale");
    if (rc) return rc;
    const uint32_t total = 9 * (Cin / 32) * (Cout / kCT) * 8 * 64;
    hipLaunchKernelGGL(conv_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w, scale,
                       Cin, Cout, su, reinterpret_cast<f4 *>(packed));
    return check_launch("conv_pack_weights: pack");
}

int sdfr_conv3x3_f16x3_ws(float *out, const void *x_split, const void *packed,
                          uint32_t B, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout,
                          int transposed, void *ws, size_t ws_bytes, void *stream) {
    if (!out) return fail(SDFR_EINVAL, "conv3x3_f16x3: null pointer");
    ConvArgs a{};
    a.out = out;
    const ConvShape s{B, H, W, Cin, Cout, transposed != 0, kEpiRaw, ws != nullptr, ws_bytes};
    return conv_run(a, s, x_split, packed, ws, (hipStream_t)stream, "conv3x3_f16x3");
}

int sdfr_conv3x3_f16x3(float *out, const void *x_split, const void *packed,
                       uint32_t B, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout,
                       int transposed, void *stream) {
    return sdfr_conv3x3_f16x3_ws(out, x_split, packed, B, H, W, Cin, Cout, transposed, nullptr, 0,
                                 stream);
}

int sdfr_set_conv_t_mode(int mode) {
    if (mode < -1 || mode > 3) return fail(SDFR_EINVAL, "set_conv_t_mode: mode must be -1..3");
    const int prev = g_conv_t_mode;
    g_conv_t_mode = mode == -1 ? conv_t_env_mode() : mode;
    return prev;
}

size_t sdfr_conv_ws_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t Cout, int transposed) {
    return plan_ws_bytes(B, H, W, Cout, transposed != 0, kEpiRaw);
}

size_t sdfr_conv_act_ws_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t Cout) {
    return plan_ws_bytes(B, H, W, Cout, false, kEpiStyled);
}

int sdfr_conv_plan(const sdfr_conv_plan_query *q, sdfr_conv_plan_info *info) {
    if (!q || !info) return fail(SDFR_EINVAL, "conv_plan: null argument");
    const ConvShape s{q->B, q->H, q->W, q->Cin, q->Cout, q->transposed != 0, q->epilogue,
                      q->has_ws != 0, q->ws_bytes};
    const ConvPlan p = plan_conv(s, g_conv_t_mode);
    *info = sdfr_conv_plan_info{};
    info->rc = p.rc;
    info->ksplit = p.ksplit;
    info->ksplit_t = p.ksplit_t;
    info->ws_bytes = p.ws_bytes;
    info->nsteps = p.nsteps;
    for (uint32_t i = 0; i < p.nsteps; ++i) {
        info->steps[i].kernel = p.steps[i].kernel;
        info->steps[i].grid_x = p.steps[i].gx;
        info->steps[i].grid_y = p.steps[i].gy;
        info->steps[i].block = p.steps[i].block;
    }
    return p.rc ? fail(p.rc, std::string("conv_plan: ") + p.msg) : SDFR_OK;
}

int sdfr_conv3x3_f16x3_act(const sdfr_conv_act_args *p, void *stream) {
    if (!p) return fail(SDFR_EINVAL, "conv3x3_f16x3_act: null args");
    const sdfr_conv_act_args &s = *p;
    if (!s.demod || !s.bias || (s.noise && !s.noise_weight))
        return fail(SDFR_EINVAL, "conv3x3_f16x3_act: null tensor pointer");
    const bool rgb = s.rgb_w || s.rgb_base;
    if (s.rgb_w && s.rgb_base) return fail(SDFR_EINVAL, "conv3x3_f16x3_act: rgb_w and rgb_base are exclusive");
    if (s.rgb_base && !s.rgb_s) return fail(SDFR_EINVAL, "conv3x3_f16x3_act: rgb_base needs rgb_s");
    if (!s.y_split && !rgb) return fail(SDFR_EINVAL, "conv3x3_f16x3_act: nothing to write");
    if (rgb && !s.rgb_partial) return fail(SDFR_EINVAL, "conv3x3_f16x3_act: rgb_partial missing");
    if (((uint64_t)s.H * s.W) % kPT)
        return fail(SDFR_EUNSUPPORTED, "conv3x3_f16x3_act: H*W must be a multiple of 256");
    // (noise: single floats in conv_x_kernel's epilogue, dword-aligned LDS-DMA pieces in
    // conv_h_kernel -- no vector load, so no 16-B rule)
    for (const void *q : {(const void *)s.demod, (const void *)s.bias, (const void *)s.s_next,
                          (const void *)s.rgb_w, (const void *)s.y_split, (const void *)s.rgb_base,
                          (const void *)s.rgb_s})
        if (q && reinterpret_cast<uintptr_t>(q) % 16)
            return fail(SDFR_EINVAL, "conv3x3_f16x3_act: pointers must be 16-B aligned");
    ConvArgs a{};
    set_act_epilogue(a.e, s.demod, s.noise, s.noise_weight, s.bias, s.negative_slope, s.act_scale,
                     s.s_next, s.y_split);
    a.e.rgb_w = s.rgb_w;
    a.e.rgbp = s.rgb_partial;
    a.e.rgb_base = s.rgb_base;
    a.e.rgb_s = s.rgb_s;
    const ConvShape sh{s.B, s.H, s.W, s.Cin, s.Cout, false, kEpiStyled, s.ws != nullptr, s.ws_bytes};
    return conv_run(a, sh, s.x_split, s.packed, s.ws, (hipStream_t)stream, "conv3x3_f16x3_act");
}

int sdfr_conv_t_act_supported(uint32_t B, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout) {
    // (a shape past the 32-bit offset limit is in range: the call refuses it, SDFR_EINVAL)
    const ConvShape s{B, H, W, Cin, Cout, true, kEpiBlur, false, 0};
    return plan_conv(s, g_conv_t_mode).rc != SDFR_EUNSUPPORTED;
}

int sdfr_conv_t_act(const sdfr_conv_t_act_args *p, void *stream) {
    if (!p) return fail(SDFR_EINVAL, "conv_t_act: null args");
    const sdfr_conv_t_act_args &s = *p;
    if (!s.demod || !s.bias || !s.y_split || !s.raw || (s.noise && !s.noise_weight))
        return fail(SDFR_EINVAL, "conv_t_act: null tensor pointer");
    // (noise too: conv_t_kernel<true> reads it with 16-B loads)
    for (const void *q : {(const void *)s.demod, (const void *)s.bias, (const void *)s.s_next,
                          (const void *)s.y_split, (const void *)s.raw, (const void *)s.noise})
        if (q && reinterpret_cast<uintptr_t>(q) % 16)
            return fail(SDFR_EINVAL, "conv_t_act: pointers must be 16-B aligned");
    ConvArgs a{};
    a.out = s.raw;
    set_act_epilogue(a.e, s.demod, s.noise, s.noise_weight, s.bias, s.negative_slope, s.act_scale,
                     s.s_next, s.y_split);
    for (int k = 0; k < 4; ++k) a.fir[k] = s.fir[k];
    const ConvShape sh{s.B, s.H, s.W, s.Cin, s.Cout, true, kEpiBlur, false, 0};
    return conv_run(a, sh, s.x_split, s.packed, nullptr, (hipStream_t)stream, "conv_t_act");
}

}  // extern "C"

// conv_common.h -- what the decoder's convolution kernels share (conv_x.h, conv_h.h,
// conv_t.h; instantiated and launched by conv_f16x3.hip): vector types, tile constants,
// the kernel argument block, the MFMA and LDS-DMA helpers, the styled epilogue's
// arithmetic, and the shared scaffolding of the halo pipeline that conv_h_kernel and
// conv_t_kernel run (the halo swizzle and DMA, a workgroup's share of the persistent
// XCD tile walk).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "conv_plan.h"   // kCT, kPT, kTCT, kCusPerXcd, ConvClass

namespace sdfr {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f2c __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kStepF4 = 1024;   // f4 of weight fragments per K-step (16 KB)
constexpr uint32_t kTStepF4 = 512;     // conv_t_kernel: f4 of weight fragments per K-step (8 KB)
// the 18 x 18 input halo of a 16 x 16 block (conv_h.h describes the image)
constexpr uint32_t kHaloW = 18;
constexpr uint32_t kHaloPx = kHaloW * kHaloW;          // 324
constexpr uint32_t kHaloPieces = 48;                  // 6 per wave; 41 carry pixels
constexpr uint32_t kHaloF4 = kHaloPieces * 64;        // 48 KB per buffer

__device__ __forceinline__ f4 mfma16(f4 a, f4 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a),
                                                  __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// Styled epilogue fused into a regular conv (sdfr_conv3x3_f16x3_act).
struct ActEpi {
    const float *demod, *noise, *noise_weight, *bias;   // [B,Cout], [B,H,W], [1], [Cout]
    float slope, scale;
    const float *s_next;           // [B,Cout] or null
    _Float16 *ys;                  // split-NHWC [B,H,W,Cout] or null
    const float *rgb_w;            // [B,3,Cout] or null
    float *rgbp;                   // [Cout/128, B, 3, H*W] ToRGB partial sums
    // or (rgb_w null) the ToRGB weight as base [3,Cout] x style [B,Cout], multiplied
    // here (the same fp32 product the caller would form: one launch less per layer)
    const float *rgb_base, *rgb_s;
};

struct ConvArgs {
    const _Float16 *xs;            // split-NHWC [B, Hin, Win, Cin/8, 2, 8]
    const f4 *wpk;                 // packed fragments (conv_f16x3.hip)
    float *out;                    // [B, Hf, Wf, Cout]
    uint32_t B, Hin, Win, Cin, Cout;
    uint32_t Hf, Wf, sy;           // full output image, class stride
    uint32_t ncls;
    ConvClass cls[4];
    int dy[9], dx[9];              // input pixel = (a + dy, c + dx)
    uint32_t tap[9];               // packed weight tap (3 ky + kx)
    ActEpi e;                      // conv_x_kernel<true> only
    uint32_t ksplit;               // split-K factor (1: the epilogue runs in the conv kernel)
    uint32_t grid;                 // workgroup slots per split (padded class tiles)
    f4 *partial;                   // [ksplit][grid][16 (i, j)][512 threads] f4 when ksplit > 1
    uint32_t tiles_t;              // conv_t_kernel: 64-channel x 16 x 16-position tiles
    uint32_t ksplit_t;             // conv_t_kernel: channel-group split of a tile (1, 2, 4)
    float *ptl;                    // ksplit_t > 1: [ksplit_t][B, Hf, Wf, Cout] partial outputs
    float fir[4];                  // conv_t_kernel<true>: the blur's 1-D taps (outer(fir, fir))
};

// Buffer resource over [base, base + bytes) (gfx950 raw buffer, range-checked).
__device__ __forceinline__ v4i make_rsrc(const void *base, uint32_t bytes) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    v4i r;
    r.x = (int)(uint32_t)b;
    r.y = (int)(uint32_t)(b >> 32);
    r.z = (int)bytes;
    r.w = 0x00020000;
    return r;
}

// One LDS-DMA piece: 64 lanes x 16 B from rsrc at (voff + soff) to LDS byte
// address lds (wave-uniform base + 16 lane).  Inline asm, so hipcc neither
// tracks it in its own s_waitcnt bookkeeping (no vmcnt(0) drain in front of
// every ds_read of the ring) nor reserves M0 across it; completion is counted
// explicitly by the ring below.  Offsets past num_records read zeros.
// M0 = LDS destination base of the following DMAs (kernel code here never uses M0
// otherwise -- checked in the ISA; the register is reserved, so it cannot be
// declared clobbered).  A DMA's instruction offset moves both its global address
// and its LDS destination, so one M0 write serves several pieces.
__device__ __forceinline__ void set_m0(uint32_t lds) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(lds) : "memory");
}
template <int IOFF>
__device__ __forceinline__ void dma16(v4i rsrc, uint32_t voff, uint32_t soff) {
    asm volatile("buffer_load_dwordx4 %0, %1, %2 offen offset:%3 lds"
                 :
                 : "v"(voff), "s"(rsrc), "s"(soff), "i"(IOFF)
                 : "memory");
}

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)reinterpret_cast<uintptr_t>(p);
}

typedef __attribute__((address_space(3))) f4 lds_f4_t;
__device__ __forceinline__ f4 lds_f4(uint32_t byte_addr) {   // LDS byte address -> f4
    return *(const lds_f4_t *)(size_t)byte_addr;
}

// keep a resource in SGPRs (the inline asm needs it there)
__device__ __forceinline__ v4i uni(v4i r) {
    return v4i{__builtin_amdgcn_readfirstlane(r.x), __builtin_amdgcn_readfirstlane(r.y),
               __builtin_amdgcn_readfirstlane(r.z), __builtin_amdgcn_readfirstlane(r.w)};
}

__device__ __forceinline__ float act1(float c, float dm, float nz, float b, float slope,
                                      float scale) {
    float v = c * dm;                  // same operation order as decoder.hip's epilogue
    v = v + nz;
    v = v + b;
    v = v > 0.0f ? v : v * slope;
    return v * scale;
}

// Round-to-nearest hi/lo split into split-NHWC (decoder.hip store_split4) for lane
// groups g = 2k, 2k+1 holding channels 4g..4g+3 of the same 8-channel group and
// pixel (lanes 16 g + n): one v_permlane16_swap per dword
// gives the even group both hi halves and the odd group both lo halves, so every
// lane issues ONE 16-B store (hi of the 8 channels at idx8, lo 16 B after it) instead
// of two 8-B stores.  idx8 = NHWC element index of the group's channel 0.  All lanes
// must execute it (cross-lane).
__device__ __forceinline__ void store_split8_pair(_Float16 *ys, size_t idx8, f4 v, uint32_t g) {
    h4 h, l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h[r] = (_Float16)v[r];
        l[r] = (_Float16)(v[r] - (float)h[r]);
    }
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    const u2 hd = __builtin_bit_cast(u2, h), ld = __builtin_bit_cast(u2, l);
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const auto r = __builtin_amdgcn_permlane16_swap(hd[k], ld[k], false, false);
        q[k] = r[0];          // even group: own hi / odd group: partner's lo
        q[2 + k] = r[1];      // even group: partner's hi / odd group: own lo
    }
    *reinterpret_cast<f4 *>(ys + 2 * idx8 + (g & 1u) * 8) = __builtin_bit_cast(f4, q);
}

// ----------------------------------------------------------------------------
// The halo pipeline's scaffolding (conv_h_kernel, conv_t_kernel).  Only what compiles
// to the same code from here as written out in the kernel: the halo source-offset loop,
// the fragment lane bases and a walk struct with advance() do not (hipcc, ROCm 7.2:
// other registers, a few instructions more or fewer), so each kernel keeps its copy.
// ----------------------------------------------------------------------------

__device__ __forceinline__ uint32_t halo_swz(uint32_t hx) { return (hx & 4u) | ((hx >> 1) & 1u); }

// One halo piece (64 lanes x 16 B at per-lane source offset hoff) of the channel group at
// soffset hsoff -> LDS at dst
__device__ __forceinline__ void halo_fire(v4i rx, const f4 *dst, uint32_t hoff, uint32_t hsoff) {
    set_m0(lds_addr(dst));
    dma16<0>(uni(rx), hoff, __builtin_amdgcn_readfirstlane(hsoff));
}

// Persistent schedule: XCD x owns items [x per, (x + 1) per) (Cout block fastest, as
// slot_tile); its workgroups take them from `first` with `stride` up to `end`, so the ones
// running together share halos and weights in the XCD's L2.  first >= end: an idle workgroup.
struct XcdShare {
    uint32_t first, stride, end;
};
__device__ __forceinline__ XcdShare xcd_share(uint32_t nitems) {
    const uint32_t per = (nitems + 7) >> 3;
    const uint32_t xcd = blockIdx.x & 7u, nwg = gridDim.x >> 3;
    const uint32_t tend = min(xcd * per + per, nitems);
    return XcdShare{(uint32_t)__builtin_amdgcn_readfirstlane(xcd * per + (blockIdx.x >> 3)), nwg, tend};
}

}  // namespace
}  // namespace sdfr

// field_pack.h -- xprep_kernel: the FiLM vectors (gamma / su) and the split-fp16 weight
// fragments of both field kernels' packings (field_r_kernel's by r_pack; layouts in
// field_common.h's K permutations).  Instantiated by field_f16x3.hip (the render's
// networks) and field_grad.hip (the gradient trunks).
#pragma once

#include "field_common.h"

namespace sdfr {

// field_r_kernel's packing (xprep_kernel): slice = one k-step of 16 K,
// [8 tiles of 32 rows][hi, lo][64 lanes], lane l holding W[32 T + (l & 31)][k] for
// k = rperm_k(layer, s, l >> 5, 0..7)
template <class Net>
__device__ __forceinline__ void r_pack(const XPrepArgs &a, uint32_t e) {
    const uint32_t slice = e / 512, rem = e % 512;
    if (slice >= (uint32_t)RNet<Net>::kSteps) return;
    const uint32_t t8 = rem >> 6, lane = rem & 63;
    int layer = 0;
    if (slice >= rslice_base<Net>(Net::kLayers - 1)) layer = Net::kLayers - 1;
    else if (slice >= (uint32_t)RNet<Net>::kL0) layer = 1 + (slice - RNet<Net>::kL0) / 16;
    const uint32_t s = slice - rslice_base<Net>(layer);
    const uint32_t row = 32 * t8 + (lane & 31), h = lane >> 5;
    const uint32_t K = Net::K(layer);
    const float sc = a.su[layer * kW + row];
    float v[8];
#pragma unroll
    for (uint32_t jj = 0; jj < 8; ++jj) {
        const int k = rperm_k<Net>(layer, s, h, jj);
        v[jj] = k < 0 ? 0.0f : __fmul_rn(a.w[layer][(size_t)row * K + k], sc);
    }
    f4 hi, lo;
    split8(v, hi, lo);
    f4 *dst = a.packed + (size_t)slice * kRSliceF4 + t8 * 128 + lane;
    dst[0] = hi;
    dst[64] = lo;
}

// blocks [0, B*films*2*256/4): FiLM rows, one wave per output row (lanes over K,
// butterfly sum); then packing, one (slice, t8, lane) per thread
template <class Net>
__global__ void __launch_bounds__(256) xprep_kernel(const XPrepArgs a) {
    constexpr int NF = Net::kFilmN;
    const uint32_t blk = blockIdx.x, j = threadIdx.x;
    const uint32_t nfilm = a.B * NF * 2 * kW / 4;
    if (blk < nfilm) {
        const uint32_t lane = j & 63u, row_id = blk * 4 + (j >> 6);
        const uint32_t jr = row_id % kW, rest = row_id / kW;
        const uint32_t b = rest / (NF * 2), rem = rest % (NF * 2);
        const uint32_t f = rem >> 1, which = rem & 1;
        const f4 s4 = reinterpret_cast<const f4 *>(a.styles + (size_t)b * kW)[lane];
        // one 256-long dot product per wave: lane l holds k = 4l .. 4l+3
        auto dot = [&](const float *W) {
            const f4 w4 = reinterpret_cast<const f4 *>(W + (size_t)jr * kW)[lane];
            float p = __fmaf_rn(s4.w, w4.w, __fmaf_rn(s4.z, w4.z, __fmaf_rn(s4.y, w4.y, __fmul_rn(s4.x, w4.x))));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) p = __fadd_rn(p, __shfl_xor(p, o));
            return p;
        };
        if constexpr (Net::kPosEnc) {
            // FCGenerator: gamma'' = 1/su (exact), beta'' = the layer bias, + style_in(s)
            // for x_in (sdf_model.py:1654-1658: x_in(p) + style_in(styles), then ReLU)
            const int l = Net::film_layer(f);
            float v;
            if (which == 0) {
                v = __fdiv_rn(1.0f, a.su[l * kW + jr]);
            } else {
                v = a.lb[l][jr];
                if (f == 0) v = __fadd_rn(v, __fadd_rn(dot(a.gw[0]), a.gb[0][jr]));
            }
            if (lane == 0) a.film[(((size_t)b * NF + f) * 2 + which) * kW + jr] = v;
            return;
        }
        const float lin = __fadd_rn(dot(which ? a.bw[f] : a.gw[f]), (which ? a.bb[f] : a.gb[f])[jr]);
        // LinearLayer: std_init * linear + bias_init (sdf_model.py:39, 58-59).  The
        // activation sin(gamma (W x + b) + beta) of the modulated layer runs as
        // sin_rev(fma(gamma'', z, beta'')) on its bias-free, row-scaled GEMM output
        // z = su W x, in revolutions: gamma'' = gamma / (su 2pi) and
        // beta'' = (gamma b + beta) / 2pi, each one correctly rounded division (in
        // double) of the reference's fp32 gamma, beta and b.  Folding the bias into
        // beta'' leaves the accumulators starting from zero (no bias rows in LDS).
        constexpr double k2pi = 6.283185307179586476925;
        const int l = Net::film_layer(f);
        float v;
        if (which) {
            // gamma of the same row (its wave is another one)
            const float g = __fadd_rn(__fmul_rn(15.0f, __fadd_rn(dot(a.gw[f]), a.gb[f][jr])), 30.0f);
            const float bet = __fadd_rn(__fmul_rn(0.25f, lin), 0.0f);
            v = (float)(((double)g * (double)a.lb[l][jr] + (double)bet) / k2pi);
        } else {
            const float gam = __fadd_rn(__fmul_rn(15.0f, lin), 30.0f);
            v = (float)((double)gam / ((double)a.su[l * kW + jr] * k2pi));
        }
        if (lane == 0) a.film[(((size_t)b * NF + f) * 2 + which) * kW + jr] = v;
        return;
    }
    const uint32_t e = (blk - nfilm) * 256 + j;
    if (e >= Net::kSlices * 512) return;
    if constexpr (Net::kFieldR) {
        r_pack<Net>(a, e);
        return;
    }
    // field_p_kernel's half-slices
    const uint32_t slice = e / 512, rem = e % 512;
    const uint32_t t8 = rem >> 6, lane = rem & 63;
    int layer = 0;
    if (slice >= xslice_base<Net>(Net::kLayers - 1)) layer = Net::kLayers - 1;
    else if (slice >= 2) layer = 1 + (slice - 2) / 16;
    const uint32_t local = slice - xslice_base<Net>(layer);
    const uint32_t q = local >> 1, h = local & 1;
    const uint32_t row = 16 * (8 * h + t8) + (lane & 15), g = lane >> 4;
    const uint32_t K = Net::K(layer);
    const float s = a.su[layer * kW + row];
    float v[8];
#pragma unroll
    for (uint32_t jj = 0; jj < 8; ++jj) {
        const int k = xperm_k<Net>(layer, q, g, jj);
        v[jj] = k < 0 ? 0.0f : __fmul_rn(a.w[layer][(size_t)row * K + k], s);
    }
    f4 hi, lo;
    split8(v, hi, lo);
    f4 *dst = a.packed + (size_t)slice * kXSliceF4 + t8 * 128 + lane;
    dst[0] = hi;
    dst[64] = lo;
}

}  // namespace sdfr

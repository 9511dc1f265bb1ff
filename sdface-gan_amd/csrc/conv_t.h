// conv_t.h -- conv_t_kernel: the stride-2 transposed convolution of an upsampling
// StyledConv (sdf_model.py:660-701, conv_transpose2d before the blur) for all four output
// parity classes of a 16 x 16 block of INPUT positions (a, c) in one workgroup, over one
// input halo per channel group (conv_h_kernel's 18 x 18 staging, anchored at
// (a - 1, c - 1)).  Class (py, px) of position (a, c) is output pixel
// (2 a + py, 2 c + px) and takes taps ky in {0, 2} (py = 0: inputs a, a - 1) or
// ky = 1 (py = 1: input a), likewise x: the four classes' 4 + 2 + 2 + 1 taps are nine
// K-steps per channel group over four input positions (dy, dx) in {0, -1}^2, ordered
// by position so a B fragment read from the halo serves every class-tap at it:
//     s    0     1     2     3  |  4     5  |  6     7  |  8
//   (ky,kx) (0,0) (0,1) (1,0) (1,1) | (2,0) (2,1) | (0,2) (1,2) | (2,2)
//   (dy,dx)        (0, 0)         |  (-1, 0)  |  (0, -1)  | (-1,-1)
// Every K-step is the same work for every wave (2 m-tiles x 4 n-tiles x 3 split terms
// into the step's class accumulators), so the nine taps of a channel group run like
// conv_h_kernel's nine: weight ring of 3 x 8 KB (64 channels x 32), halo of the next
// group fired over the first six steps, one barrier per step, persistent tiles.
// conv_x_kernel staged 256 shifted pixels per tap and ran each class as its own
// workgroups (a 1-tap class: 8-16 K-steps per 128 KB of fp32 stores).
// Output: the raw fp32 (2H + 1)^2 grid for rows / columns < 2H, 2W; the last row and
// column (even classes at a = H, c = W) are four thin classes of conv_x_kernel.
#pragma once

#include "conv_common.h"

namespace sdfr {
namespace {

__host__ __device__ constexpr int t_ky(int s) {
    return (s == 2 || s == 3 || s == 7) ? 1 : ((s == 4 || s == 5 || s == 8) ? 2 : 0);
}
__host__ __device__ constexpr int t_kx(int s) { return s < 6 ? (s & 1) : 2; }
__host__ __device__ constexpr int t_pos(int s) { return s < 4 ? 0 : (s < 6 ? 1 : (s < 8 ? 2 : 3)); }

// ---- conv_t_kernel<true>: the upsampling StyledConv's blur and styled epilogue ----
// (sdf_model.py:674-683, 704-818: Blur(pad (1, 1), 4 x 4 = outer(fir, fir)) of the
// transposed conv's (2H + 1)^2 output, then demod, noise, bias, leaky ReLU x sqrt 2 and
// the next layer's modulation; epi_blur_kernel's arithmetic, in its order).  A block's
// 32 x 32 output pixels need its 35 x 35 conv outputs (one row / column before, two
// after): the interior 29 x 29 are finished here from the accumulators -- the 4-tap
// horizontal pass across lanes (DPP row shifts within the 16-lane rows that hold a
// position row's 16 columns), the vertical pass across a lane's rows, the rows at the
// 4-row wave boundaries exchanged through LDS -- and the border pixels (rows and
// columns 0, 30, 31 of a block) by conv_t_border_kernel, from the raw conv values of
// the band rows / columns (0-2, 29-31) that this kernel stores instead of the whole
// fp32 output.
__device__ __forceinline__ bool t_band(uint32_t r) { return r <= 2u || r >= 29u; }
__device__ __forceinline__ bool t_border(uint32_t r) { return r == 0u || r >= 30u; }

// value of lane n - 1 (PREV) or n + 1 of the lane's 16-lane row; 0 past the row's end.
// (The whole vector is bit-cast: hipcc (ROCm 7.2) reads element 0 for a bit_cast of one
// element v[k] of an ext-vector, whatever k -- DESIGN.md §5.2.)
template <bool PREV>
__device__ __forceinline__ f4 dpp_row_shift(f4 v) {
    typedef int i4 __attribute__((ext_vector_type(4)));
    constexpr int ctl = PREV ? 0x111 : 0x101;           // row_shr:1 / row_shl:1
    const i4 iv = __builtin_bit_cast(i4, v);
    i4 r;
    r.x = __builtin_amdgcn_update_dpp(0, iv.x, ctl, 0xF, 0xF, true);
    r.y = __builtin_amdgcn_update_dpp(0, iv.y, ctl, 0xF, 0xF, true);
    r.z = __builtin_amdgcn_update_dpp(0, iv.z, ctl, 0xF, 0xF, true);
    r.w = __builtin_amdgcn_update_dpp(0, iv.w, ctl, 0xF, 0xF, true);
    return __builtin_bit_cast(f4, r);
}

// store_split8_pair, the store only where `live` (both lanes of a pair agree on it)
__device__ __forceinline__ void store_split8_pair_if(_Float16 *ys, size_t idx8, f4 v, uint32_t g,
                                                     bool live) {
    asm volatile("" : "+v"(v));        // the fp32 product rounded first (not folded into the cvt)
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
        uint32_t r0 = r[0], r1 = r[1];
        asm volatile("" : "+v"(r0), "+v"(r1));
        q[k] = r0;
        q[2 + k] = r1;
    }
    if (live) *reinterpret_cast<f4 *>(ys + 2 * idx8 + (g & 1u) * 8) = __builtin_bit_cast(f4, q);
}

// 4-tap filter in epi_blur_kernel's order: fma chain from 0 (horizontal, hfilt) ...
__device__ __forceinline__ f4 fir_h(const f4 &v0, const f4 &v1, const f4 &v2, const f4 &v3,
                                    float f0, float f1, float f2, float f3) {
    f4 h;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        h[k] = fmaf(v3[k], f3, fmaf(v2[k], f2, fmaf(v1[k], f1, fmaf(v0[k], f0, 0.0f))));
    return h;
}
// ... and from the first product (vertical)
__device__ __forceinline__ f4 fir_v(const f4 &h0, const f4 &h1, const f4 &h2, const f4 &h3,
                                    float f0, float f1, float f2, float f3) {
    f4 s;
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = fmaf(h3[k], f3, fmaf(h2[k], f2, fmaf(h1[k], f1, h0[k] * f0)));
    return s;
}

// The epilogue of one conv_t_kernel<true> tile.  acc[2 py + px][i][j]: channels
// 16 (2 wm + i) + 4 g .. + 3 of the block's 64, input position (4 wn + j, n), output pixel
// (2 (4 wn + j) + py, 2 n + px) of the block.  Ep: the tile's demod, bias, s_next (64
// channels, f4 0-15 of pieces 0-2) and noise (32 x 32 floats from f4 192), staged at the
// tile's start (conv_t_kernel); Xs: 48 KB of LDS free during the epilogue (the halo
// buffer of odd channel groups).  No global load here: one issued behind the epilogue's
// stores would wait for them to drain (vmcnt retires in order).
__device__ __forceinline__ void conv_t_blur_epilogue(const ConvArgs &a0, f4 (&acc)[4][2][4],
                                                     const f4 *Ep, f4 *Xs, uint32_t lane,
                                                     uint32_t wave, uint32_t cb, uint32_t b,
                                                     uint32_t y0, uint32_t x0) {
    asm volatile("" : "+v"(lane), "+s"(wave));
    const ConvArgs &a = a0;
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    const uint32_t n = lane & 15u, g = lane >> 4;
    const uint32_t C = a.Cout, Wf = a.Wf, H2 = 2u * a.Hin, W2 = 2u * a.Win;
    const ActEpi &e = a.e;
    const size_t pbase = (size_t)b * H2 + 2u * y0;
    const float nw = e.noise ? *e.noise_weight : 0.0f;   // (a scalar load)
    const float *epn = reinterpret_cast<const float *>(Ep + 192);
    // 1. the raw conv values of the band rows / columns (conv_t_border_kernel's input)
    {
        float *raw = a.out + (size_t)cb * kTCT + 2u * wm * 16u + 4u * g;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t yr = 2u * (4u * wn + j) + (uint32_t)(q >> 1);
                const uint32_t xr = 2u * n + (uint32_t)(q & 1);
                if (t_band(yr) || t_band(xr)) {
                    float *dst = raw + ((size_t)(b * a.Hf + 2u * y0 + yr) * Wf + 2u * x0 + xr) * C;
#pragma unroll
                    for (int i = 0; i < 2; ++i) *reinterpret_cast<f4 *>(dst + i * 16) = acc[q][i][j];
                }
            }
    }
    const float f0 = a.fir[3], f1 = a.fir[2], f2 = a.fir[1], f3 = a.fir[0];   // flipped taps
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // the K loop's reads of Xs are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // per 16-channel m-tile (register pressure)
        // (scheduling fences: left free, hipcc hoists m-tile 1's DPP reads above m-tile
        // 0's stores and spills them; a scratch reload behind the stores waits for them)
        __builtin_amdgcn_sched_barrier(0);
        // 2. horizontal pass in place: acc[2 py + px] <- conv row 2 a + py filtered at
        //    column 2 c + px (columns 2c-1 .. 2c+2: lane n - 1's px 1, own px 0 / 1, lane
        //    n + 1's px 0 / 1)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                const f4 c0 = acc[2 * py][i][j], c1 = acc[2 * py + 1][i][j];
                const f4 l1 = dpp_row_shift<true>(c1);
                const f4 r0 = dpp_row_shift<false>(c0), r1 = dpp_row_shift<false>(c1);
                acc[2 * py][i][j] = fir_h(l1, c0, c1, r0, f0, f1, f2, f3);
                acc[2 * py + 1][i][j] = fir_h(c0, c1, r0, r1, f0, f1, f2, f3);
            }
        __builtin_amdgcn_sched_barrier(0);
        // 3. rows across the 4-row wave boundaries: wave (wm, wn) needs row 4 wn - 1's
        //    odd conv row (wave - 2's j = 3, py = 1) and row 4 wn + 4's two (wave + 2's
        //    j = 0).  (A barrier separates the previous m-tile's reads from these writes.)
        if (i) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        f4 *mine = Xs + wave * 6u * 64u + lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) mine[q * 64] = acc[q][i][0];
        mine[4 * 64] = acc[2][i][3];
        mine[5 * 64] = acc[3][i][3];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // (read where used: wave - 2's rows for j = 0, wave + 2's for j = 3; the top and
        // bottom waves read a neighbour's slot of no use -- those pixels are borders)
        const f4 *above = Xs + ((wave - 2u) & 7u) * 6u * 64u + lane;
        const f4 *below = Xs + ((wave + 2u) & 7u) * 6u * 64u + lane;
        // 4. vertical pass, styled epilogue, split store (interior pixels)
        const uint32_t lq = (2u * wm + i) * 4u + g;         // f4 index of the channel quad
        const uint32_t ch = cb * kTCT + 4u * lq;
        const f4 dm = Ep[lq], bs = Ep[64 + lq], sn = Ep[128 + lq];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const f4 hm1 = j > 0 ? acc[2 + px][i][j - 1] : above[(4 + px) * 64];  // a - 1, py 1
                const f4 h00 = acc[px][i][j], h01 = acc[2 + px][i][j];                 // a, py 0 / 1
                const f4 hp0 = j < 3 ? acc[px][i][j + 1] : below[px * 64];            // a + 1, py 0
                const f4 hp1 = j < 3 ? acc[2 + px][i][j + 1] : below[(2 + px) * 64];  // a + 1, py 1
#pragma unroll
                for (int py = 0; py < 2; ++py) {
                    const f4 sv = py == 0 ? fir_v(hm1, h00, h01, hp0, f0, f1, f2, f3)
                                          : fir_v(h00, h01, hp0, hp1, f0, f1, f2, f3);
                    const uint32_t yr = 2u * (4u * wn + j) + py, xr = 2u * n + px;
                    const float nz = nw * epn[yr * 32u + xr];
                    f4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = act1(sv[r], dm[r], nz, bs[r], e.slope, e.scale);
                    const size_t P = (pbase + yr) * W2 + 2u * x0 + xr;
                    store_split8_pair_if(e.ys, P * C + (ch & ~7u), v * sn, g,
                                         !t_border(yr) && !t_border(xr));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
    }
}

// The border pixels of conv_t_kernel<true>'s blocks (rows and columns 0, 30 and 31 of
// every 32 x 32 output block: their blur reaches a neighbouring block's conv outputs),
// from the raw band rows / columns and the edge classes' last row / column in a.out,
// with epi_blur_kernel's arithmetic.  The border pixels come in runs of three across
// each block boundary (rows / columns 32 k - 2 .. 32 k); a thread takes one channel
// quad of either a row run x 4 adjacent columns (6 x 7 raw values for 12 outputs) or a
// column run in one non-border row (4 x 6 raw values for 3 outputs).
__device__ __forceinline__ f4 border_ld(const float *src, int yy, int xx, uint32_t Hi, uint32_t Wi,
                                        uint32_t C) {
    return (yy >= 0 && yy < (int)Hi && xx >= 0 && xx < (int)Wi)
               ? *reinterpret_cast<const f4 *>(src + ((size_t)yy * Wi + xx) * C)
               : f4{0.0f, 0.0f, 0.0f, 0.0f};
}

__device__ __forceinline__ void border_out(const ConvArgs &a, uint32_t b, uint32_t Y, uint32_t X,
                                           uint32_t c, f4 s, const f4 &dm, const f4 &bs,
                                           const f4 &sn, float nw) {
    const ActEpi &e = a.e;
    const uint32_t C = a.Cout, H2 = 2u * a.Hin, W2 = 2u * a.Win;
    const size_t P = ((size_t)b * H2 + Y) * W2 + X;
    const float nz = e.noise ? nw * e.noise[P] : 0.0f;
    f4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act1(s[r], dm[r], nz, bs[r], e.slope, e.scale);
    v = v * sn;
    asm volatile("" : "+v"(v));
    h4 hh, ll;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        hh[r] = (_Float16)v[r];
        ll[r] = (_Float16)(v[r] - (float)hh[r]);
    }
    const size_t idx = P * C + c, o = 2 * idx - (idx & 7u);
    *reinterpret_cast<h4 *>(e.ys + o) = hh;
    *reinterpret_cast<h4 *>(e.ys + o + 8) = ll;
}

template <bool ROWS>
__global__ void __launch_bounds__(256) conv_t_border_kernel(const ConvArgs a) {
    const uint32_t Q = a.Cout >> 2, H2 = 2u * a.Hin, W2 = 2u * a.Win;
    const uint32_t kb = H2 / 32u + 1u, mb = W2 / 32u + 1u;      // row / column boundaries
    const uint32_t items = ROWS ? kb * (W2 / 4u) : (H2 / 4u) * mb;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)a.B * items * Q) return;
    const uint32_t q = (uint32_t)(t % Q);
    const uint64_t r1 = t / Q;
    const uint32_t item = (uint32_t)(r1 % items);
    const uint32_t b = (uint32_t)(r1 / items);
    const uint32_t c = 4u * q, C = a.Cout, Hi = a.Hf, Wi = a.Wf;
    const float *src = a.out + (size_t)b * Hi * Wi * C + c;
    const float f0 = a.fir[3], f1 = a.fir[2], f2 = a.fir[1], f3 = a.fir[0];
    const ActEpi &e = a.e;
    const f4 dm = *reinterpret_cast<const f4 *>(e.demod + (size_t)b * C + c);
    const f4 bs = *reinterpret_cast<const f4 *>(e.bias + c);
    const f4 sn = e.s_next ? *reinterpret_cast<const f4 *>(e.s_next + (size_t)b * C + c)
                           : f4{1.0f, 1.0f, 1.0f, 1.0f};
    const float nw = e.noise ? *e.noise_weight : 0.0f;
    if constexpr (ROWS) {
        // output rows 32 k - 2 .. 32 k (those inside the image) x columns X0 .. X0 + 3
        const uint32_t k = item / (W2 / 4u), X0 = 4u * (item % (W2 / 4u));
        const int Yb = 32 * (int)k - 2;
        // rows Yb - 1 .. Yb + 4 one at a time (a 4-row window of filtered rows: VGPRs)
        f4 h[4][4];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            f4 v[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) v[j] = border_ld(src, Yb - 1 + r, (int)X0 - 1 + j, Hi, Wi, C);
#pragma unroll
            for (int x = 0; x < 4; ++x)
                h[r & 3][x] = fir_h(v[x], v[x + 1], v[x + 2], v[x + 3], f0, f1, f2, f3);
            if (r >= 3) {
                const int y = r - 3, Y = Yb + y;
                if (Y >= 0 && Y < (int)H2) {
#pragma unroll
                    for (int x = 0; x < 4; ++x)
                        border_out(a, b, (uint32_t)Y, X0 + x, c,
                                   fir_v(h[y & 3][x], h[(y + 1) & 3][x], h[(y + 2) & 3][x],
                                         h[(y + 3) & 3][x], f0, f1, f2, f3),
                                   dm, bs, sn, nw);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // rows 4 r .. 4 r + 3 (the non-border ones: 1 .. 29 of a block) x output columns
        // 32 m - 2 .. 32 m, rows one at a time through a 4-row window
        const uint32_t m = item % mb, Y0 = 4u * (item / mb);
        const int Xb = 32 * (int)m - 2;
        f4 h[4][3];
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            f4 v[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = border_ld(src, (int)Y0 - 1 + r, Xb - 1 + j, Hi, Wi, C);
#pragma unroll
            for (int x = 0; x < 3; ++x)
                h[r & 3][x] = fir_h(v[x], v[x + 1], v[x + 2], v[x + 3], f0, f1, f2, f3);
            if (r >= 3) {
                const int y = r - 3;
                const uint32_t Y = Y0 + y, yb = Y & 31u;
                if (yb != 0u && yb < 30u) {
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        const int X = Xb + x;
                        if (X < 0 || X >= (int)W2) continue;
                        border_out(a, b, Y, (uint32_t)X, c,
                                   fir_v(h[y & 3][x], h[(y + 1) & 3][x], h[(y + 2) & 3][x],
                                         h[(y + 3) & 3][x], f0, f1, f2, f3),
                                   dm, bs, sn, nw);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <bool FUSE>
__global__ void __launch_bounds__(512, 1) conv_t_kernel(const ConvArgs a) {
    __shared__ f4 As[3][kTStepF4];       // weight ring [mt 4][hi,lo][64]
    __shared__ f4 Hs[2][kHaloF4];        // halo images, by channel-group parity
    __shared__ f4 Ep[FUSE ? 7 * 64 : 1]; // FUSE: the tile's epilogue operands
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    const uint32_t H = a.Hin, W = a.Win;
    const uint32_t nC = a.Cin / 32, nB = a.Cout / kCT, nT = a.Cout / kTCT;
    const uint32_t nbx = W / 16, nby = H / 16;
    const v4i rw = make_rsrc(a.wpk, 9u * nC * nB * kStepF4 * 16u);
    const v4i rx = make_rsrc(a.xs, a.B * H * W * a.Cin * 4);
    // tile -> 64-channel block cb, image b, block origin (y0, x0); this wave's halo
    // pieces k = wave + 8 i (per-lane source offsets at channel group 0)
    // work item = (tile, K split): the split's channel groups [cg0, cg1)
    const uint32_t ks = a.ksplit_t;
    uint32_t cb = 0, bimg = 0, y0 = 0, x0 = 0, split = 0, cg0 = 0, cg1 = 0, hoff[6];
    auto setup = [&](uint32_t item) {
        uint32_t ln = lane, wv = wave;        // opaque: computed here, not hoisted
        asm volatile("" : "+v"(ln), "+s"(wv));
        const uint32_t tile = item / ks;
        split = item - tile * ks;
        cg0 = split * nC / ks;
        cg1 = (split + 1) * nC / ks;
        cb = tile % nT;
        uint32_t blk = tile / nT;
        const uint32_t bx = blk % nbx;
        blk /= nbx;
        const uint32_t by = blk % nby, b = blk / nby;
        bimg = b;
        y0 = by * 16;
        x0 = bx * 16;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint32_t h = 8u * (wv + 8u * i) + (ln >> 3);
            const uint32_t hy = h / kHaloW, hx = h - hy * kHaloW;
            const uint32_t q = (ln & 7u) ^ halo_swz(hx);
            const int y = (int)(y0 + hy) - 1, x = (int)(x0 + hx) - 1;
            const bool ok = h < kHaloPx && y >= 0 && y < (int)H && x >= 0 && x < (int)W;
            hoff[i] = ok ? (((b * H + (uint32_t)y) * W + (uint32_t)x) * a.Cin * 4u + q * 16u)
                         : 0x7FFFFFF0u;
        }
    };
    uint32_t c0 = 0, c1 = 0;              // the running item's channel groups
    const uint32_t n = lane & 15u, g = lane >> 4;
    // B fragment lane bases (bytes within a halo buffer): [column offset dx + 1][lo]
    uint32_t fb0[2][2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int lo = 0; lo < 2; ++lo)
            fb0[d][lo] = (4u * wn * kHaloW + n) * 128u + (((2u * g + lo) ^ halo_swz(n + d)) << 4);
    const uint32_t hs0 = lds_addr(&Hs[0][0]), hs1 = lds_addr(&Hs[1][0]);

    // weights of K-step S of group c (tap 3 ky + kx): this block's 4 m-tiles are 8 KB,
    // one 1 KB piece per wave
    auto fire_w = [&](uint32_t c, auto sc, uint32_t stage) {
        constexpr int S = decltype(sc)::value;
        constexpr uint32_t tap = 3 * t_ky(S) + t_kx(S);
        const uint32_t wsoff = __builtin_amdgcn_readfirstlane(
            ((tap * nC + c) * nB + (cb >> 1)) * kStepF4 * 16u + (cb & 1u) * kTStepF4 * 16u +
            wave * 1024u);
        set_m0(lds_addr(&As[stage][wave * 64]));
        dma16<0>(uni(rw), lane * 16u, wsoff);
    };
    uint32_t hsoff = 0;                   // soffset of the group being fetched (c * 128 B)
    auto fire_h = [&](int buf, int i) {
        halo_fire(rx, &Hs[buf][(wave + 8u * i) * 64], hoff[i], hsoff);
    };
    f4 acc[4][2][4];                      // [class 2 py + px][m-tile i][n-tile j]
    f4 Aset[2][4];                        // [hi i0, hi i1, lo i0, lo i1] by step parity
    f4 Bset[2][8];                        // [hi j0..3, lo j0..3] by position parity
    auto read_a = [&](f4 (&A)[4], uint32_t st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            A[i] = As[st][((2 * wm + i) * 2) * 64 + lane];
            A[2 + i] = As[st][((2 * wm + i) * 2 + 1) * 64 + lane];
        }
    };
    auto read_b = [&](f4 (&Bf)[8], auto posc, uint32_t hs) {
        constexpr int pos = decltype(posc)::value;
        constexpr uint32_t dyp = (pos == 1 || pos == 3) ? 0 : 1, dxp = pos >= 2 ? 0 : 1;
        const uint32_t bh = hs + fb0[dxp][0], bl = hs + fb0[dxp][1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t imm = ((j + dyp) * kHaloW + dxp) * 128u;
            Bf[j] = lds_f4(bh + imm);
            Bf[4 + j] = lds_f4(bl + imm);
        }
    };
    // split term t (0: lo.hi, 1: hi.lo, 2: hi.hi) of m-tile i into class cl
    auto mfma_quad = [&](auto clc, const f4 (&A)[4], const f4 (&Bf)[8], int i, int t) {
        constexpr int cl = decltype(clc)::value;
        const f4 &ra = t == 0 ? A[2 + i] : A[i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[cl][i][j] = mfma16(ra, t == 1 ? Bf[4 + j] : Bf[j], acc[cl][i][j]);
    };

    auto prologue = [&] {
        hsoff = cg0 * 128u;
#pragma unroll
        for (int i = 0; i < 6; ++i) fire_h(0, i);
        hsoff += 128u;
        fire_w(cg0, std::integral_constant<int, 0>{}, 0);
        fire_w(cg0, std::integral_constant<int, 1>{}, 1);
        fire_w(cg0, std::integral_constant<int, 2>{}, 2);
    };

    // persistent schedule: this workgroup's share of the tiles_t * ks items
    const XcdShare sh = xcd_share(a.tiles_t * ks);
    const uint32_t nwg = sh.stride, tend = sh.end;
    uint32_t tile = sh.first;
    if (tile >= tend) return;
    uint32_t next = tile + nwg;
    bool has_next = next < tend;

    // K-step (c, S): MFMAs of m-tile 0; wait (in flight may stay only what step -1
    // fired: its weight piece and halo piece); barrier; read step +1's A fragments and,
    // at a position change, its B fragments; MFMAs of m-tile 1 with step +3's weight
    // piece and (S <= 5) a halo piece of group c + 1 between the split terms.  PAR:
    // parity of group c (its halo buffer and the fragment sets), compile-time.
    auto step = [&](uint32_t c, auto sc, auto parc) {
        constexpr int S = decltype(sc)::value, PAR = decltype(parc)::value;
        constexpr int cl = 2 * (t_ky(S) & 1) + (t_kx(S) & 1);
        constexpr int ka = (9 * PAR + S) & 1, kb = (4 * PAR + t_pos(S)) & 1;
        f4 (&A)[4] = Aset[ka];
        f4 (&An)[4] = Aset[ka ^ 1];
        f4 (&Bf)[8] = Bset[kb];
        f4 (&Bn)[8] = Bset[kb ^ 1];
        const auto CL = std::integral_constant<int, cl>{};
        const uint32_t k = (c - c0) * 9 + S, nk = (c1 - c0) * 9;
        const bool prev_w = k + 2 < nk;
        const bool prev_h = S != 0 && S - 1 <= 5 && c + 1 < c1;
        mfma_quad(CL, A, Bf, 0, 0);
        mfma_quad(CL, A, Bf, 0, 1);
        mfma_quad(CL, A, Bf, 0, 2);
        if (prev_w && prev_h) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        else if (prev_w || prev_h) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        read_a(An, (S + 1) % 3);
        if constexpr (S == 3 || S == 5 || S == 7)
            read_b(Bn, std::integral_constant<int, t_pos(S + 1)>{}, PAR ? hs1 : hs0);
        else if constexpr (S == 8)
            read_b(Bn, std::integral_constant<int, 0>{}, PAR ? hs0 : hs1);
        mfma_quad(CL, A, Bf, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (k + 3 < nk)
            fire_w(c + (S + 3) / 9, std::integral_constant<int, (S + 3) % 9>{}, S % 3);
        __builtin_amdgcn_sched_barrier(0);
        mfma_quad(CL, A, Bf, 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (S <= 5) {
            if (c + 1 < c1) fire_h(1 - PAR, S);
        }
        if constexpr (S == 8) {
            if (k + 1 == nk && has_next) {
                setup(next);
                prologue();
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_quad(CL, A, Bf, 1, 2);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto group = [&](uint32_t c, auto parc) {
        step(c, std::integral_constant<int, 0>{}, parc);
        step(c, std::integral_constant<int, 1>{}, parc);
        step(c, std::integral_constant<int, 2>{}, parc);
        step(c, std::integral_constant<int, 3>{}, parc);
        step(c, std::integral_constant<int, 4>{}, parc);
        step(c, std::integral_constant<int, 5>{}, parc);
        hsoff += 128u;
        step(c, std::integral_constant<int, 6>{}, parc);
        step(c, std::integral_constant<int, 7>{}, parc);
        step(c, std::integral_constant<int, 8>{}, parc);
    };

    setup(tile);
    prologue();
    bool first = true;
    for (;;) {
        const uint32_t ecb = cb, eb = bimg, ey0 = y0, ex0 = x0, esp = split;  // (setup moves on)
        c0 = cg0;
        c1 = cg1;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[q][i][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        // everything but step 2's weight piece (and, after the first tile, the previous
        // epilogue's 32 stores, younger than this tile's prologue) has landed; the
        // epilogue reads no LDS.  FUSE: its stores and loads vary per lane -- wait for
        // them all (as conv_h_kernel); its LDS exchange is done everywhere after the barrier.
        // FUSE: the tile's epilogue operands, one 1 KB piece per wave 0-6 -- demod, bias,
        // s_next (the block's 64 channels in lanes 0-15), the noise of its 32 x 32 output
        // pixels (8 rows per wave) -- loaded here, where the wait below drains the
        // previous epilogue's stores anyway, and written to Ep behind the barrier
        f4 epv = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (FUSE) {
            const ActEpi &e = a.e;
            const uint32_t ln = lane;
            const uint32_t ch = cb * kTCT + 4u * (ln & 15u);
            const bool lo = ln < 16u;
            const f4 *src = nullptr;
            if (wave == 0) src = lo ? reinterpret_cast<const f4 *>(e.demod + (size_t)bimg * a.Cout + ch) : nullptr;
            else if (wave == 1) src = lo ? reinterpret_cast<const f4 *>(e.bias + ch) : nullptr;
            else if (wave == 2) src = lo && e.s_next ? reinterpret_cast<const f4 *>(e.s_next + (size_t)bimg * a.Cout + ch) : nullptr;
            else if (wave < 7 && e.noise)
                src = reinterpret_cast<const f4 *>(
                    e.noise + ((size_t)bimg * 2u * H + 2u * y0 + 8u * (wave - 3u) + (ln >> 3)) * 2u * W +
                    2u * x0 + 4u * (ln & 7u));
            if (src) epv = *src;
            else if (wave == 2) epv = f4{1.0f, 1.0f, 1.0f, 1.0f};
        }
        if (first && !FUSE) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        else if (FUSE) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(33) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if constexpr (FUSE) {
            if (wave < 7) Ep[wave * 64 + lane] = epv;
        }
        read_a(Aset[0], 0);
        read_b(Bset[0], std::integral_constant<int, 0>{}, hs0);
        uint32_t c = c0;
        for (; c + 1 < c1; c += 2) {
            group(c, std::integral_constant<int, 0>{});
            group(c + 1, std::integral_constant<int, 1>{});
        }
        if (c < c1) group(c, std::integral_constant<int, 0>{});
        if constexpr (FUSE) {
            conv_t_blur_epilogue(a, acc, Ep, &Hs[1][0], lane, wave, ecb, eb, ey0, ex0);
        } else {   // raw fp32 outputs of the four classes
            uint32_t ln = lane, wmm = wm, wnn = wn;   // opaque: nothing hoisted into the K loop
            asm volatile("" : "+v"(ln), "+s"(wmm), "+s"(wnn));
            const uint32_t nn = ln & 15u, gg = ln >> 4;
            const uint32_t Wf = a.Wf, C = a.Cout;
            // (a K split writes its partial output; conv_t_finish_kernel sums them)
            float *base = (ks > 1 ? a.ptl + (size_t)esp * a.B * a.Hf * Wf * C : a.out) + ecb * kTCT +
                          4u * gg;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t oy = 2u * (ey0 + 4u * wnn + j) + (uint32_t)(q >> 1);
                    const uint32_t ox = 2u * (ex0 + nn) + (uint32_t)(q & 1);
                    float *dst = base + ((size_t)(eb * a.Hf + oy) * Wf + ox) * C;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        *reinterpret_cast<f4 *>(dst + (2u * wmm + i) * 16u) = acc[q][i][j];
                }
        }
        if (!has_next) break;
        tile = next;
        next = tile + nwg;
        has_next = next < tend;
        first = false;
    }
}

// conv_t_kernel's K-split finish: out = sum of the ksplit_t partials, in split order
// (deterministic), for every output row / column < 2H, 2W (the edge classes write theirs)
__global__ void __launch_bounds__(256) conv_t_finish_kernel(const ConvArgs a) {
    const uint32_t C4 = a.Cout / 4, W2 = 2 * a.Win, H2 = 2 * a.Hin;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)a.B * H2 * W2 * C4) return;
    const uint32_t q = (uint32_t)(t % C4);
    uint64_t r = t / C4;
    const uint32_t ox = (uint32_t)(r % W2);
    r /= W2;
    const uint32_t oy = (uint32_t)(r % H2), b = (uint32_t)(r / H2);
    const size_t idx = (((size_t)b * a.Hf + oy) * a.Wf + ox) * a.Cout + 4 * q;
    const size_t stride = (size_t)a.B * a.Hf * a.Wf * a.Cout;
    f4 v = *reinterpret_cast<const f4 *>(a.ptl + idx);
    for (uint32_t k = 1; k < a.ksplit_t; ++k) v += *reinterpret_cast<const f4 *>(a.ptl + k * stride + idx);
    *reinterpret_cast<f4 *>(a.out + idx) = v;
}

}  // namespace
}  // namespace sdfr

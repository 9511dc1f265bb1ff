// conv_x.h -- conv_x_kernel, the strip kernel of the decoder's 3x3 convolutions: any
// class of output pixels (the regular conv's one, the transposed conv's four parity
// classes, conv_t_kernel's thin edge classes) as an implicit GEMM, with its epilogue
// and its split-K finish.
//
// Workgroup: 128 output channels x 256 output pixels, 8 waves of 64 x 64 (two per
// SIMD), K in steps of 32 input channels at one tap.  Both operands arrive
// already split (weights pre-packed in fragment order; activations in the
// split-NHWC layout the previous epilogue writes, 32 channels of a pixel's hi and
// lo = one 128-B line) and are staged global -> LDS by LDS-DMA (buffer_load ...
// lds: no VGPRs, no VALU; the buffer range check zero-fills the padding taps)
// through a 3-stage ring of 48 KB stages: two K-steps stay in flight behind a
// counted vmcnt and a raw barrier, one workgroup per CU.  The workgroup order is
// XCD-aware, and the four parity classes of a transposed conv share one launch.
#pragma once

#include "conv_common.h"

namespace sdfr {
namespace {

constexpr int kStages = 3;   // LDS-DMA ring depth (kStages - 1 K-steps in flight)

// Epilogue of one workgroup tile: raw fp32 output (NHWC, class pixel placement) or,
// with ACT, the fused styled epilogue (sdfr_conv3x3_f16x3_act).
template <bool ACT>
__device__ __forceinline__ void conv_epilogue(const ConvArgs &a, f4 (&acc)[4][4], uint32_t lane,
                                              uint32_t wm, uint32_t wn, uint32_t cb, uint32_t pix0,
                                              uint32_t npix, uint32_t Hc, uint32_t Wc, uint32_t py,
                                              uint32_t px, uint32_t rs = 16, uint32_t a0 = 0,
                                              uint32_t c0 = 0) {
    // epilogue: lane (n, g) of tile (i, j) holds channels 16 mt + 4 g .. +3 of pixel 16 nt + n
    const uint32_t n = lane & 15u, g = lane >> 4;
    if constexpr (ACT) {
        // Styled epilogue on the accumulators (regular conv, H W % 256 == 0: one face
        // per workgroup): v = lrelu(acc demod + nw noise + bias) scale; y = v s_next
        // as split-NHWC; ToRGB partial over this workgroup's 128 channels -> rgbp.
        // n-tile row r = 4 wn + j holds pixels pix0 + r rs + n (rs = 16: a 256-pixel
        // strip; rs = W: a 16 x 16 block, conv_h_kernel).
        __shared__ float red[4][4][16][3];          // [wn][j][n][o] from the wm = 1 waves
        const ActEpi &e = a.e;
        const uint32_t HW = Hc * Wc, b = pix0 / HW;
        const float nw = e.noise ? *e.noise_weight : 0.0f;
        float part[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j][0] = part[j][1] = part[j][2] = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t ch = cb * kCT + (4 * wm + i) * 16 + 4 * g;
            const f4 dm = *reinterpret_cast<const f4 *>(e.demod + (size_t)b * a.Cout + ch);
            const f4 bs = *reinterpret_cast<const f4 *>(e.bias + ch);
            const f4 sn = e.s_next ? *reinterpret_cast<const f4 *>(e.s_next + (size_t)b * a.Cout + ch)
                                   : f4{1.0f, 1.0f, 1.0f, 1.0f};
            f4 rw[3];
            const f4 rsty = e.rgb_base ? *reinterpret_cast<const f4 *>(e.rgb_s + (size_t)b * a.Cout + ch)
                                       : f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int o = 0; o < 3; ++o)
                rw[o] = e.rgb_w ? *reinterpret_cast<const f4 *>(e.rgb_w + ((size_t)b * 3 + o) * a.Cout + ch)
                      : e.rgb_base ? *reinterpret_cast<const f4 *>(e.rgb_base + (size_t)o * a.Cout + ch) * rsty
                                   : f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t P = pix0 + (4 * wn + j) * rs + n;
                const float nz = e.noise ? nw * e.noise[P] : 0.0f;
                f4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = act1(acc[i][j][r], dm[r], nz, bs[r], e.slope, e.scale);
                if (e.ys) store_split8_pair(e.ys, (size_t)P * a.Cout + (ch & ~7u), v * sn, g);
#pragma unroll
                for (int o = 0; o < 3; ++o)
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[j][o] = fmaf(v[r], rw[o][r], part[j][o]);
            }
        }
        if (e.rgb_w || e.rgb_base) {
            // sum over the 4 channel groups g (lanes n + 16 g), then over wm (LDS)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    part[j][o] += __shfl_xor(part[j][o], 16, 64);
                    part[j][o] += __shfl_xor(part[j][o], 32, 64);
                }
            if (wm == 1 && g == 0)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int o = 0; o < 3; ++o) red[wn][j][n][o] = part[j][o];
            __syncthreads();
            if (wm == 0 && g < 3) {                 // lane (n, g = o) stores channel o
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t P = pix0 + (4 * wn + j) * rs + n;
                    const float s = (g == 0 ? part[j][0] : g == 1 ? part[j][1] : part[j][2]) +
                                    red[wn][j][n][g];
                    e.rgbp[(((size_t)cb * a.B + b) * 3 + g) * HW + (P - b * HW)] = s;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t P = pix0 + (4 * wn + j) * 16 + n;
        if (P >= npix) continue;
        const uint32_t hw = Hc * Wc;
        const uint32_t b = P / hw, rem = P % hw;
        const uint32_t oy = a.sy * (rem / Wc + a0) + py, ox = a.sy * (rem % Wc + c0) + px;
        float *dst = a.out + (((size_t)b * a.Hf + oy) * a.Wf + ox) * a.Cout + cb * kCT + 4 * g;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f4 *>(dst + (4 * wm + i) * 16) = acc[i][j];
    }
}

// Workgroup slot -> (class, tile); false for a padding slot.  Class ranges start at
// multiples of 8, so slot % 8 is the XCD.
__device__ __forceinline__ bool slot_tile(const ConvArgs &a, uint32_t slot, uint32_t &ci,
                                          uint32_t &tile) {
    ci = 0;
    for (uint32_t i = 1; i < a.ncls; ++i)
        if (slot >= a.cls[i].tile0) ci = i;
    const ConvClass &cl = a.cls[ci];
    const uint32_t loc = slot - cl.tile0;
    // XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs; give
    // each XCD one contiguous run of the class's tiles, with the Cout block fastest,
    // so the tiles that re-read an activation row (the other Cout blocks of the same
    // pixels, the rows above and below through the taps) run on the same XCD at
    // about the same time and hit its L2.  (The K splits of a slot, blockIdx.y, sit
    // on the same XCD: the grid's x extent is a multiple of 8.)
    tile = (loc & 7u) * ((cl.ntiles + 7) >> 3) + (loc >> 3);
    return tile < cl.ntiles;
}

template <bool ACT>
__global__ void __launch_bounds__(512, 1) conv_x_kernel(const ConvArgs a) {
    __shared__ f4 As[kStages][kStepF4];       // [mt 8][hi,lo][64]
    __shared__ f4 Bs[kStages][2 * kStepF4];   // [nt 16][hi,lo][64]
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    uint32_t ci, tile;
    if (!slot_tile(a, blockIdx.x, ci, tile)) return;  // padding slot (whole workgroup)
    const ConvClass &cl = a.cls[ci];
    const uint32_t Hc = cl.Hc, Wc = cl.Wc, py = cl.py, px = cl.px;
    const uint32_t ntaps = cl.ntaps;
    const uint32_t npix = a.B * Hc * Wc;
    const uint32_t nC = a.Cin / 32, nB = a.Cout / kCT;
    const uint32_t cb = tile % nB;
    const uint32_t pix0 = (tile / nB) * kPT;
    // split-K: blockIdx.y's share of the class's K-steps (channel group x tap)
    const uint32_t nk_all = nC * ntaps, split = blockIdx.y;
    const uint32_t k_begin = split * nk_all / a.ksplit, nk = (split + 1) * nk_all / a.ksplit - k_begin;

    // LDS-DMA sources (6 pieces of 1 KB per wave per K-step).  Weights: the K-step's
    // 16 KB block is contiguous; wave w moves pieces 2w, 2w+1.  Activations: the 32
    // channels of one pixel are one 128-B line of the split-NHWC input
    // ([g 4][hi 8, lo 8] halves); a piece is 8 pixels = 8 whole lines, region
    // (nt, half) of n-tile nt = pixels 16 nt + 8 half .. +7.  Lane l fetches pixel
    // l & 7, channel group g = (l >> 3) & 3, plane h = l >> 5 to LDS unit l, so a
    // region holds [h][g][pixel] and the fragment read below is conflict-free.
    // Wave w moves regions (2w, 0..1) and (2w+1, 0..1).
    const uint32_t xbytes = a.B * a.Hin * a.Win * a.Cin * 4;
    const v4i rw = make_rsrc(a.wpk, 9u * nC * nB * kStepF4 * 16u);
    const v4i rx = make_rsrc(a.xs, xbytes);
    const uint32_t loff = ((lane >> 3) & 3u) * 32u + (lane >> 5) * 16u;
    // per tap (8-bit descriptors, SGPRs): packed weight tap, dy, dx
    const uint32_t td0 = cl.td[0], td1 = cl.td[1], td2 = cl.td[2];
    auto tapdesc = [&](uint32_t t) -> uint32_t {
        const uint32_t w = t < 4 ? td0 : (t < 8 ? td1 : td2);
        return (w >> (8 * (t & 3u))) & 0xFFu;
    };
    // Per activation piece: the lane's own input offset (its output pixel at dy = dx
    // = 0, + channel group / plane) and a bit per tap telling whether the tap's
    // input pixel exists (zero padding otherwise): the K loop then needs one add
    // and one select per piece, all tap arithmetic being uniform (SALU).
    uint32_t xoff[4], tmask[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t P = pix0 + (2 * wave + (k >> 1)) * 16 + (k & 1) * 8 + (lane & 7u);
        const bool pv = P < npix;
        const uint32_t Pc = pv ? P : 0;
        const uint32_t hw = Hc * Wc;
        const uint32_t pb = Pc / hw, rem = Pc % hw, pa = rem / Wc + cl.a0, pc = rem % Wc + cl.c0;
        xoff[k] = ((pb * a.Hin + pa) * a.Win + pc) * a.Cin * 4u + loff;
        uint32_t m = 0;
        for (uint32_t t = 0; t < ntaps; ++t) {
            const uint32_t d = tapdesc(t);
            const int iy = (int)pa + (int)((d >> 4) & 3u) - 1, ix = (int)pc + (int)(d >> 6) - 1;
            if (pv && iy >= 0 && iy < (int)a.Hin && ix >= 0 && ix < (int)a.Win) m |= 1u << t;
        }
        tmask[k] = m;
    }

    // K-step issue order is sequential (0, 1, 2 in the prologue, then ks + 3 at
    // step ks): (channel group, tap) advance incrementally
    // The address work (SALU tap decode, VALU offsets) is done in prep_step, ahead
    // of the barrier and overlapped with MFMAs; fire_step after the barrier only
    // moves M0 and issues the six DMAs.
    uint32_t nx_c = k_begin / ntaps, nx_t = k_begin % ntaps;
    struct StepDma {
        uint32_t wsoff;           // weight pieces: global offset of this wave's first
        uint32_t offs[4];         // activation pieces: per-lane global offsets
    };
    auto prep_step = [&]() -> StepDma {
        StepDma r;
        const uint32_t c = nx_c, tl = nx_t;
        const bool wrap = nx_t + 1 == ntaps;
        nx_t = wrap ? 0u : nx_t + 1;
        nx_c = wrap ? nx_c + 1 : nx_c;
        const uint32_t d = tapdesc(tl);
        const uint32_t wbase = (((d & 15u) * nC + c) * nB + cb) * kStepF4 * 16u;
        r.wsoff = wbase + 2 * wave * 1024u;
        const int dy = (int)((d >> 4) & 3u) - 1, dx = (int)(d >> 6) - 1;
        const uint32_t toff = (uint32_t)((dy * (int)a.Win + dx) * (int)a.Cin * 4) + c * 128u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = (tmask[k] >> tl) & 1u;
            r.offs[k] = ok ? xoff[k] + toff : 0x7FFFFFF0u;   // past num_records: zero fill
        }
        return r;
    };
    auto fire_step = [&](const StepDma &r, uint32_t buf) {
        set_m0(lds_addr(&As[buf][2 * wave * 64]));
        dma16<0>(rw, lane * 16u, r.wsoff);
        dma16<1024>(rw, lane * 16u, r.wsoff);
        // (one M0 per piece: an instruction offset would move the -- per-lane, possibly
        // small -- global offsets too)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            set_m0(lds_addr(&Bs[buf][(4 * wave + k) * 64]));
            dma16<0>(rx, r.offs[k], 0u);
        }
    };
    auto issue_step = [&](uint32_t ks, uint32_t buf) {
        (void)ks;
        fire_step(prep_step(), buf);
    };

    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};

    // Fragments of one K-step: [0..3] A hi, [4..7] A lo, [8..11] B hi, [12..15] B lo.
    // B lane (g = lane >> 4, n = lane & 15): region (nt, n >> 3), unit h 32 + 8 g + (n & 7).
    const uint32_t boff = ((lane >> 3) & 1u) * 64u + (lane >> 4) * 8u + (lane & 7u);
    auto read_frags = [&](f4 (&R)[16], uint32_t st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            R[i] = As[st][((4 * wm + i) * 2) * 64 + lane];
            R[4 + i] = As[st][((4 * wm + i) * 2 + 1) * 64 + lane];
            R[8 + i] = Bs[st][((4 * wn + i) * 2) * 64 + boff];
            R[12 + i] = Bs[st][((4 * wn + i) * 2) * 64 + boff + 32];
        }
    };
    // rows i0 .. i0+nr-1 of the wave's 4 x 4 tiles; per A fragment the three split
    // terms sweep the 4 B fragments (consecutive MFMAs never share an accumulator)
    auto mfma_rows = [&](const f4 (&R)[16], int i0, int nr) {
#pragma unroll
        for (int i = i0; i < i0 + nr; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(R[4 + i], R[8 + j], acc[i][j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(R[i], R[12 + j], acc[i][j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(R[i], R[8 + j], acc[i][j]);
        }
    };

    // Ring: step ks lives in stage ks % 3 and is read into registers half a step
    // early.  Half-way through step ks (rows 0-1 done) the wave waits for its pieces
    // of step ks+1 (ks+2's 6 may stay in flight), drains its LDS reads and meets the
    // others at a raw barrier: after it step ks+1 is in LDS everywhere and nobody
    // reads stage ks % 3 any more, so step ks+3 is issued into it and step ks+1's
    // fragments are read while rows 2-3 of step ks compute.
    uint32_t st_ks = 0;
    auto step = [&](uint32_t ks, const f4 (&R)[16], f4 (&Rn)[16]) {
        const bool fire = ks + kStages < nk;
        const bool more = kStages == 3 && ks + 2 < nk;
        StepDma pr = prep_step();                   // (counters advance past nk harmlessly)
        // materialise the DMA addresses here, in the MFMA shadow (the compiler would
        // otherwise sink them past the barrier into the issue block)
        asm volatile("" : "+s"(pr.wsoff));
#pragma unroll
        for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(pr.offs[k]));
        mfma_rows(R, 0, 2);
        if (more) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const uint32_t st = st_ks, st1 = st_ks == kStages - 1 ? 0u : st_ks + 1;
        st_ks = st1;                                   // ks % kStages, carried
        if (fire) fire_step(pr, st);
        if (ks + 1 < nk) read_frags(Rn, st1);
        mfma_rows(R, 2, 2);
    };
    issue_step(0, 0);
    if (nk > 1) issue_step(1, 1);
    if (kStages == 3 && nk > 2) issue_step(2, 2);
    if (kStages == 3 && nk > 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (nk > 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    f4 R0[16], R1[16];
    read_frags(R0, 0);
    uint32_t ks = 0;
    for (; ks + 1 < nk; ks += 2) {
        step(ks, R0, R1);
        step(ks + 1, R1, R0);
    }
    if (ks < nk) step(ks, R0, R1);

    if (a.ksplit > 1) {      // partial sums; conv_splitk_kernel adds them and runs the epilogue
        f4 *pp = a.partial + ((size_t)split * a.grid + blockIdx.x) * 16 * 512 + tid;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) pp[(i * 4 + j) * 512] = acc[i][j];
        return;
    }
    conv_epilogue<ACT>(a, acc, lane, wm, wn, cb, pix0, npix, Hc, Wc, py, px, 16, cl.a0, cl.c0);
}

// Split-K finish: the ksplit partial tiles summed in split order (deterministic),
// then the tile's epilogue, with the conv kernel's slot -> tile mapping and lane
// roles.  Used when the unsplit grid would leave CUs idle (eval.py's batch of 1:
// 64 workgroups at 64^2, 128 at 128^2, for 256 CUs).
template <bool ACT>
__global__ void __launch_bounds__(512, 1) conv_splitk_kernel(const ConvArgs a) {
    uint32_t ci, tile;
    if (!slot_tile(a, blockIdx.x, ci, tile)) return;
    const ConvClass &cl = a.cls[ci];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    const uint32_t nB = a.Cout / kCT, cb = tile % nB, pix0 = (tile / nB) * kPT;
    // every split's 16 f4 loaded before the first add (all 64 loads in flight)
    f4 acc[4][4], t[3][16];
    const f4 *pp = a.partial + (size_t)blockIdx.x * 16 * 512 + tid;
    const size_t sstride = (size_t)a.grid * 16 * 512;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = pp[(i * 4 + j) * 512];
#pragma unroll
    for (uint32_t s = 1; s < 4; ++s)
        if (s < a.ksplit)
#pragma unroll
            for (int q = 0; q < 16; ++q) t[s - 1][q] = pp[s * sstride + q * 512];
#pragma unroll
    for (uint32_t s = 1; s < 4; ++s)
        if (s < a.ksplit)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += t[s - 1][i * 4 + j];
    conv_epilogue<ACT>(a, acc, lane, wm, wn, cb, pix0, a.B * cl.Hc * cl.Wc, cl.Hc, cl.Wc, cl.py,
                       cl.px, 16, cl.a0, cl.c0);
}

}  // namespace
}  // namespace sdfr

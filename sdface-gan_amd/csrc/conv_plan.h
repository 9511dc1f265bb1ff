// conv_plan.h -- every host-side decision of the decoder convolutions, as data.
//
// plan_conv() turns a shape, an epilogue kind, the offered workspace and the conv_t mode
// into a ConvPlan: the refusal (code and message) or the tap and class tables, the split
// factors, the workspace bytes at which the chosen path takes its split, and the launch
// steps.  conv_f16x3.hip executes a plan; its size and support queries read one.  Plain
// C++17 with no HIP in it, so the dispatch can be checked on a host without a GPU
// (sdfr_conv_plan, tests/test_host.py).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/sdfr.h"

namespace sdfr {

constexpr int kCT = 128;        // output channels per workgroup
constexpr int kPT = 256;        // output pixels per workgroup
constexpr uint32_t kTCT = 64;          // output channels per conv_t workgroup
constexpr uint32_t kCusPerXcd = 32;   // MI355X: 256 CUs in 8 XCDs (persistent grids)
// one 128 x 256 fp32 partial tile of a split-K pass: [16 (i, j)][512 threads] f4
constexpr size_t kPartialTileBytes = 16 * 512 * 16;

// One output-pixel class: the plain convolution has one (every pixel, 9 taps); the
// stride-2 transposed one has four parity classes (4, 2, 2 and 1 taps) that share
// one launch, heaviest first, so their tails overlap.
struct ConvClass {
    uint32_t Hc, Wc;               // the class's output grid
    uint32_t py, px;               // output pixel (a, c) -> (sy (a + a0) + py, sy (c + c0) + px)
    uint32_t a0, c0;               // grid origin (0; conv_t_kernel's edge rows / columns)
    uint32_t ntaps, t0;            // its taps: dy/dx/tap[t0 .. t0 + ntaps)
    uint32_t tile0, ntiles;        // workgroups [tile0, tile0 + pad8(ntiles)) of the grid
    uint32_t td[3];                // tap descriptors, 8 bits per tap (tap | dy+1 << 4 | dx+1 << 6)
};

enum ConvEpilogue : int {
    kEpiRaw = SDFR_CONV_EPI_RAW,         // fp32 NHWC output (sdfr_conv3x3_f16x3[_ws])
    kEpiStyled = SDFR_CONV_EPI_STYLED,   // sdfr_conv3x3_f16x3_act (regular conv)
    kEpiBlur = SDFR_CONV_EPI_BLUR,       // sdfr_conv_t_act (transposed conv)
};

struct ConvShape {
    uint32_t B, H, W, Cin, Cout;
    bool transposed;
    int epi;                       // ConvEpilogue
    bool has_ws;                   // a workspace is offered ...
    size_t ws_bytes;               // ... of this size
};

enum ConvKernel : uint32_t {
    kKConvX = SDFR_CONV_K_X,                      // conv_x_kernel<false>
    kKConvXAct = SDFR_CONV_K_X_ACT,               // conv_x_kernel<true>
    kKSplitK = SDFR_CONV_K_SPLITK,                // conv_splitk_kernel<false>
    kKSplitKAct = SDFR_CONV_K_SPLITK_ACT,         // conv_splitk_kernel<true>
    kKConvH = SDFR_CONV_K_H,                      // conv_h_kernel<false>
    kKConvHSplit = SDFR_CONV_K_H_SPLIT,           // conv_h_kernel<true>
    kKConvHFinish = SDFR_CONV_K_H_FINISH,         // conv_h_finish_kernel
    kKConvT = SDFR_CONV_K_T,                      // conv_t_kernel<false>
    kKConvTFuse = SDFR_CONV_K_T_FUSE,             // conv_t_kernel<true>
    kKConvTFinish = SDFR_CONV_K_T_FINISH,         // conv_t_finish_kernel
    kKBorderRows = SDFR_CONV_K_T_BORDER_ROWS,     // conv_t_border_kernel<true>
    kKBorderCols = SDFR_CONV_K_T_BORDER_COLS,     // conv_t_border_kernel<false>
};

struct ConvStep {
    uint32_t kernel;               // ConvKernel
    uint32_t gx, gy, block;        // grid (x, y) and workgroup size
};
constexpr uint32_t kMaxConvSteps = SDFR_CONV_PLAN_MAX_STEPS;

struct ConvPlan {
    int rc;                        // SDFR_OK, or the refusal ...
    const char *msg;               // ... and its message (the caller names the entry point)
    uint32_t Hf, Wf, sy;           // full output image, class stride
    uint32_t ncls, ntap;
    ConvClass cls[4];
    int dy[9], dx[9];              // input pixel = (a + dy, c + dx)
    uint32_t tap[9];               // packed weight tap (3 ky + kx)
    uint32_t grid;                 // conv_x_kernel's workgroup slots per split (padded class tiles)
    uint32_t ksplit;               // split-K factor of conv_x_kernel / conv_h_kernel (1: none)
    uint32_t tiles_t;              // conv_t_kernel: 64-channel x 16 x 16-position tiles
    uint32_t ksplit_t;             // conv_t_kernel: channel-group split of a tile (1, 2, 4)
    size_t ws_bytes;               // the workspace from which the path takes its split (0: it has none)
    uint32_t nsteps;
    ConvStep steps[kMaxConvSteps];
};

// split-K factor: the largest of 4, 3, 2 that keeps the split grid within ~1.25 rounds
// of workgroups on the 256 CUs (one 512-thread workgroup per CU).  The 1.25: the
// batch-1 64 -> 128 transposed conv (136 workgroups, four unequal parity classes)
// measured 82 -> 66 us with a 2-way split over 272 (a one-round bound leaves it unsplit);
// 384 made the regular convs' 3-way splits slower.
constexpr uint32_t kKsplitMax = 320;
inline uint32_t conv_ksplit(uint32_t grid) {
    for (uint32_t k = 4; k > 1; --k)
        if (grid * k <= kKsplitMax) return k;
    return 1;
}

// a persistent kernel's grid (conv_h_kernel, conv_t_kernel): up to one workgroup per CU,
// a multiple of 8 (XCD count)
inline uint32_t conv_h_grid(uint32_t ntiles) {
    const uint32_t per = (ntiles + 7) >> 3;
    return 8u * (per < kCusPerXcd ? per : kCusPerXcd);
}

inline ConvPlan plan_refuse(ConvPlan p, int rc, const char *msg) {
    p.rc = rc;
    p.msg = msg;
    p.nsteps = 0;
    return p;
}

inline void plan_step(ConvPlan &p, ConvKernel k, uint32_t gx, uint32_t gy, uint32_t block) {
    p.steps[p.nsteps++] = ConvStep{k, gx, gy, block};
}

inline void plan_tap(ConvPlan &p, int ky, int kx, bool transposed) {
    p.dy[p.ntap] = transposed ? -(ky >> 1) : ky - 1;
    p.dx[p.ntap] = transposed ? -(kx >> 1) : kx - 1;
    p.tap[p.ntap] = (uint32_t)(ky * 3 + kx);
    ++p.ntap;
}

// A class over the last nt taps added: a contiguous workgroup range padded to a multiple
// of 8 (slot % 8 is the XCD).
inline void plan_class(ConvPlan &p, const ConvShape &s, uint32_t Hc, uint32_t Wc, uint32_t py,
                       uint32_t px, uint32_t nt, uint32_t a0 = 0, uint32_t c0 = 0) {
    ConvClass &c = p.cls[p.ncls++];
    c.Hc = Hc;
    c.Wc = Wc;
    c.py = py;
    c.px = px;
    c.a0 = a0;
    c.c0 = c0;
    c.t0 = p.ntap - nt;
    c.ntaps = nt;
    c.tile0 = p.grid;
    c.ntiles = (s.B * Hc * Wc + kPT - 1) / kPT * (s.Cout / kCT);
    p.grid += (c.ntiles + 7) & ~7u;
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t d = p.tap[c.t0 + t] | (uint32_t)(p.dy[c.t0 + t] + 1) << 4 |
                           (uint32_t)(p.dx[c.t0 + t] + 1) << 6;
        c.td[t >> 2] |= d << (8 * (t & 3u));
    }
}

// The transposed conv on conv_t_kernel: every output row / column < 2H, 2W there; the last
// row (even classes at a = H: only the ky = 2 taps reach it) and column as four thin
// classes of conv_x_kernel (~70 tiles at 32 faces, each a full-K loop; splitting their K
// measured slower), then for the fused blur the blocks' border pixels.
inline void plan_conv_t(ConvPlan &p, const ConvShape &s) {
    const uint32_t B = s.B, H = s.H, W = s.W, Cout = s.Cout;
    const bool fuse = s.epi == kEpiBlur;
    plan_tap(p, 2, 0, true), plan_tap(p, 2, 2, true);
    plan_class(p, s, 1, W + 1, 0, 0, 2, H, 0);       // row 2H, even columns
    plan_tap(p, 2, 1, true);
    plan_class(p, s, 1, W, 0, 1, 1, H, 0);           // row 2H, odd columns
    plan_tap(p, 0, 2, true), plan_tap(p, 2, 2, true);
    plan_class(p, s, H, 1, 0, 0, 2, 0, W);           // column 2W, even rows < 2H
    plan_tap(p, 1, 2, true);
    plan_class(p, s, H, 1, 1, 0, 1, 0, W);           // column 2W, odd rows
    plan_step(p, fuse ? kKConvTFuse : kKConvT, conv_h_grid(p.tiles_t * p.ksplit_t), 1, 512);
    if (p.ksplit_t > 1) {
        const uint64_t n4 = (uint64_t)B * 4 * H * W * (Cout / 4);
        plan_step(p, kKConvTFinish, (uint32_t)((n4 + 255) / 256), 1, 256);
    }
    plan_step(p, kKConvX, p.grid, 1, 512);
    if (fuse) {        // after the edge classes, whose last row / column they read
        const uint32_t H2 = 2u * H, W2 = 2u * W;
        const uint64_t nr = (uint64_t)B * (H2 / 32u + 1u) * (W2 / 4u) * (Cout / 4u);
        const uint64_t nc = (uint64_t)B * (H2 / 4u) * (W2 / 32u + 1u) * (Cout / 4u);
        plan_step(p, kKBorderRows, (uint32_t)((nr + 255) / 256), 1, 256);
        plan_step(p, kKBorderCols, (uint32_t)((nc + 255) / 256), 1, 256);
    }
}

// The strip kernel (conv_x_kernel) or, for the styled regular conv on 16 x 16 blocks,
// conv_h_kernel; split-K over the offered workspace when the grid would leave CUs idle.
inline void plan_strips(ConvPlan &p, const ConvShape &s) {
    const bool act = s.epi == kEpiStyled;
    const uint32_t ks = conv_ksplit(p.grid);
    p.ws_bytes = ks > 1 ? (size_t)ks * p.grid * kPartialTileBytes : 0;
    if (s.has_ws && ks > 1 && s.ws_bytes >= p.ws_bytes) p.ksplit = ks;
    if (act && s.H % 16 == 0 && s.W % 16 == 0) {
        // conv_h_kernel's split takes whole channel groups (the same K ranges as
        // conv_x_kernel's split-K when nC % ks == 0): the largest factor <= conv_ksplit's
        // that divides the group count
        while (p.ksplit > 1 && (s.Cin / 32) % p.ksplit) --p.ksplit;
        const uint32_t nt = p.cls[0].ntiles;
        if (p.ksplit > 1) {
            plan_step(p, kKConvHSplit, conv_h_grid(nt * p.ksplit), 1, 512);
            plan_step(p, kKConvHFinish, nt, 4, 128);
        } else {
            plan_step(p, kKConvH, conv_h_grid(nt), 1, 512);
        }
        return;
    }
    plan_step(p, act ? kKConvXAct : kKConvX, p.grid, p.ksplit, 512);
    if (p.ksplit > 1) plan_step(p, act ? kKSplitKAct : kKSplitK, p.grid, 1, 512);
}

// mode: the process-wide conv_t mode (sdfr_set_conv_t_mode).  1 takes conv_t_kernel for a
// transposed conv with 16-aligned input from 256 tiles (one per CU; smaller batches keep
// conv_x_kernel's split-K), 0 never (A/B measurements), 2 at any tile count (tests), 3 as
// 2 and splits each tile's channel groups 4 or 2 ways below 256 tiles when the workspace
// holds the partial outputs (measured slower than conv_x_kernel's split-K at one face: its
// thin edge-class launch alone is a 29 us serial chain there).
inline ConvPlan plan_conv(const ConvShape &s, int mode) {
    ConvPlan p{};
    p.ksplit = p.ksplit_t = 1;
    const uint32_t B = s.B, H = s.H, W = s.W, Cin = s.Cin, Cout = s.Cout;
    const bool blur = s.epi == kEpiBlur;
    const char *below = "shape below conv_t_kernel's range (sdfr_conv_t_act_supported)";
    if (s.epi < kEpiRaw || s.epi > kEpiBlur || (blur && !s.transposed) ||
        (s.epi == kEpiStyled && s.transposed))
        return plan_refuse(p, SDFR_EINVAL, "the epilogue does not go with this conv form");
    if (B == 0 || H == 0 || W == 0 || Cout % kCT || Cin % 32 || Cin == 0 || Cout == 0)
        return blur ? plan_refuse(p, SDFR_EUNSUPPORTED, below)
                    : plan_refuse(p, SDFR_EINVAL, "bad shape (Cout % 128, Cin % 32)");
    const uint64_t tiles = (uint64_t)B * (H / 16) * (W / 16) * (Cout / kTCT);
    const bool conv_t = s.transposed && mode != 0 && H % 16 == 0 && W % 16 == 0 &&
                        (tiles >= 256 || mode >= 2);
    if (blur && !conv_t) return plan_refuse(p, SDFR_EUNSUPPORTED, below);
    p.Hf = s.transposed ? 2 * H + 1 : H;
    p.Wf = s.transposed ? 2 * W + 1 : W;
    p.sy = s.transposed ? 2 : 1;
    if ((uint64_t)B * H * W * Cin * 4 >= (1ull << 31) || 9ull * Cin * Cout * 4 >= (1ull << 31) ||
        (uint64_t)B * H * W * Cout * 4 >= (1ull << 31) ||
        (blur && (uint64_t)B * p.Hf * p.Wf * Cout * 4 >= (1ull << 31)))
        return plan_refuse(p, SDFR_EINVAL, "tensor too large for 32-bit offsets (split B)");
    if (conv_t) {
        p.tiles_t = (uint32_t)tiles;
        if (mode == 3 && !blur && tiles < 256) {
            // the partial outputs of the widest split the tile count allows (for any Cin:
            // an upper bound); the split itself also wants 2 k channel groups
            for (uint32_t k = 4; k > 1 && p.ws_bytes == 0; k /= 2)
                if (tiles * k <= 256) p.ws_bytes = (size_t)k * B * p.Hf * p.Wf * Cout * sizeof(float);
            for (uint32_t k = 4; k > 1 && p.ksplit_t == 1; k /= 2)
                if (s.has_ws && s.ws_bytes >= p.ws_bytes && tiles * k <= 256 && Cin / 32 >= 2 * k)
                    p.ksplit_t = k;
        }
        plan_conv_t(p, s);
    } else if (s.transposed) {
        // conv_transpose2d, stride 2: out (2a + ky, 2c + kx) <- x (a, c).  Parity class
        // (py, px): output (2a' + py, 2c' + px) takes ky in {0, 2} (py = 0, input row
        // a' - ky/2) or ky = 1 (py = 1, input row a'), likewise for x.
        for (uint32_t py = 0; py < 2; ++py)
            for (uint32_t px = 0; px < 2; ++px) {
                uint32_t nt = 0;
                for (int ky = (int)py; ky < 3; ky += 2)
                    for (int kx = (int)px; kx < 3; kx += 2, ++nt) plan_tap(p, ky, kx, true);
                plan_class(p, s, py ? H : H + 1, px ? W : W + 1, py, px, nt);
            }
        plan_strips(p, s);
    } else {
        for (int t = 0; t < 9; ++t) plan_tap(p, t / 3, t % 3, false);
        plan_class(p, s, H, W, 0, 0, 9);
        plan_strips(p, s);
    }
    return p;
}

}  // namespace sdfr

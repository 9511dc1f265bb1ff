// conv_h.h -- conv_h_kernel: the regular 3x3 convolution with the styled epilogue, on
// 16 x 16 pixel blocks whose 18 x 18 input halo is staged ONCE per channel group and read
// at the nine tap offsets (conv_x_kernel stages every tap's 256 shifted pixels:
// 9 x 32 KB of activations per channel group against 41 KB here; with the 16 KB of
// weights per K-step the L2 -> LDS stream per K-step drops from 48 KB to ~21 KB).
//
// Halo image per channel group: [hy 18][hx 18] pixels of 128 B (the group's 32
// channels as split-NHWC quads q = 2 g + lo), quad q stored at slot q ^ swz(hx)
// with swz(hx) = (hx & 4) | (hx >> 1 & 1): the 16 lanes of every ds_read_b128
// lane group then hit 16 distinct bank quads whatever the tap's column shift
// (checked exhaustively for all shifts).  The LDS-DMA applies the swizzle through
// each lane's source address (a piece's destinations are fixed: 8 consecutive
// image pixels).  Zero padding: out-of-image lanes read past num_records.
// A fragment address is a per-lane base (one of 3 column shifts x hi/lo, plus the
// buffer) and a compile-time offset (row and column of the tap and n-tile), so the
// unrolled tap loop reads fragments without address VALU.  The weight ring and the
// mid-step barrier / next-step fragment schedule are conv_x_kernel's;
// the nine taps of a channel group are unrolled (stage = tap % 3), two groups per
// loop iteration so the register sets alternate.
//
// Persistent: one workgroup per CU (LDS 155 KB) walks a strided share of its XCD's
// contiguous tile run.  After the last K-step's barrier every LDS buffer is free, so
// the NEXT tile's prologue (halo of channel group 0, weights of its first three
// K-steps) is issued there and lands under the last MFMAs and this tile's epilogue,
// instead of behind a workgroup exit + dispatch + cold prologue.  The epilogue's
// per-channel operands (demod, bias, s_next, ToRGB weights) and the block's noise
// arrive in LDS by six more DMA pieces during the tile's second K-step, so the
// epilogue issues no global load that would have to wait (in-order vmcnt) behind the
// next tile's DMAs.
#pragma once

#include "conv_common.h"
#include "conv_x.h"   // conv_epilogue<true> (conv_h_finish_kernel)

namespace sdfr {
namespace {

// epilogue operand pieces (1 KB, one per wave 0..6): demod, bias, s_next (128
// channels in lanes 0-31 each), ToRGB weights o = 0 | 1, o = 2 (the face's rows of
// rgb_w, or rgb_base's), noise (16 rows x 16), the face's rgb_s row (rgb_base only)
constexpr uint32_t kEpPieces = 7;

// conv_epilogue<true> for a 16 x 16 block whose epilogue operands sit in LDS (Ep):
// same arithmetic in the same order; lane (n, g) of tile (i, j) holds channels
// 16 (4 wm + i) + 4 g .. +3 of block pixel (row 4 wn + j, column n).
__device__ __forceinline__ void conv_h_epilogue(const ConvArgs &a, f4 (&acc)[4][4], const f4 *Ep,
                                                uint32_t lane, uint32_t wm, uint32_t wn,
                                                uint32_t cb, uint32_t pix0, uint32_t b) {
    __shared__ float red[4][4][16][3];          // [wn][j][n][o] from the wm = 1 waves
    // opaque copies: nothing of the epilogue's address arithmetic is hoisted out of
    // conv_h_kernel's tile loop (it would stay live through the K loop and spill)
    asm volatile("" : "+v"(lane), "+s"(wm), "+s"(wn));
    uint32_t W = a.Win, HW = a.Hin * a.Win;
    asm volatile("" : "+s"(W), "+s"(HW));
    const uint32_t n = lane & 15u, g = lane >> 4;
    const ActEpi &e = a.e;
    const float nw = e.noise ? *e.noise_weight : 0.0f;
    const float *epn = reinterpret_cast<const float *>(Ep + 5 * 64);
    float part[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) part[j][0] = part[j][1] = part[j][2] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lq = (4 * wm + i) * 4 + g;     // f4 index of the channel quad
        const uint32_t ch = cb * kCT + 4 * lq;
        const f4 dm = Ep[lq], bs = Ep[64 + lq];
        const f4 sn = e.s_next ? Ep[128 + lq] : f4{1.0f, 1.0f, 1.0f, 1.0f};
        f4 rw[3] = {Ep[192 + lq], Ep[224 + lq], Ep[256 + lq]};
        if (e.rgb_base) {                               // base rows x the face's style
            const f4 rs = Ep[384 + lq];
#pragma unroll
            for (int o = 0; o < 3; ++o) rw[o] = rw[o] * rs;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = 4 * wn + j;
            const uint32_t P = pix0 + r * W + n;
            const float nz = e.noise ? nw * epn[r * 16 + n] : 0.0f;
            f4 v;
            // packed fp32 (two channels per v_pk_* op, each the same IEEE operation
            // in the same order as act1: bit-identical; no MFMA runs beside the
            // epilogue, where packed fp32 would cost issue slots)
#pragma unroll
            for (int hp = 0; hp < 2; ++hp) {
                const f2c c2 = {acc[i][j][2 * hp], acc[i][j][2 * hp + 1]};
                f2c u = c2 * f2c{dm[2 * hp], dm[2 * hp + 1]};
                u = u + f2c{nz, nz};
                u = u + f2c{bs[2 * hp], bs[2 * hp + 1]};
                const f2c neg = u * f2c{e.slope, e.slope};
                u = f2c{u.x > 0.0f ? u.x : neg.x, u.y > 0.0f ? u.y : neg.y};
                u = u * f2c{e.scale, e.scale};
                v[2 * hp] = u.x;
                v[2 * hp + 1] = u.y;
            }
            if (e.ys) store_split8_pair(e.ys, (size_t)P * a.Cout + (ch & ~7u), v * sn, g);
            // channels o = 0, 1 of the ToRGB partials as one packed chain (the same
            // fma per element, the same q order), o = 2 alone
            f2c p01 = {part[j][0], part[j][1]};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                p01 = __builtin_elementwise_fma(f2c{v[q], v[q]}, f2c{rw[0][q], rw[1][q]}, p01);
                part[j][2] = fmaf(v[q], rw[2][q], part[j][2]);
            }
            part[j][0] = p01.x;
            part[j][1] = p01.y;
        }
    }
    if (e.rgb_w || e.rgb_base) {
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
        // raw barrier: the LDS writes above are all it orders (a __syncthreads fence
        // could add a vmcnt wait on the next tile's DMAs)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wm == 0 && g < 3) {                 // lane (n, g = o) stores channel o
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t P = pix0 + (4 * wn + j) * W + n;
                const float s = (g == 0 ? part[j][0] : g == 1 ? part[j][1] : part[j][2]) +
                                red[wn][j][n][g];
                e.rgbp[(((size_t)cb * a.B + b) * 3 + g) * HW + (P - b * HW)] = s;
            }
        }
        // red is rewritten by the next tile's epilogue only after that tile's barriers
    }
}

template <bool SPLIT>
__global__ void __launch_bounds__(512, 1) conv_h_kernel(const ConvArgs a) {
    __shared__ f4 As[3][kStepF4];        // weight ring [mt 8][hi,lo][64]
    __shared__ f4 Hs[2][kHaloF4];        // halo images, by channel-group parity
    __shared__ f4 Ep[kEpPieces * 64];    // epilogue operands of the current tile
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    const uint32_t H = a.Hin, W = a.Win;
    const uint32_t nC = a.Cin / 32, nB = a.Cout / kCT;
    const uint32_t nbx = W / 16, nby = H / 16;
    const v4i rw = make_rsrc(a.wpk, 9u * nC * nB * kStepF4 * 16u);
    const v4i rx = make_rsrc(a.xs, a.B * H * W * a.Cin * 4);
    // tile -> Cout block cb, first pixel pix0 (image b, block origin y0, x0) and this
    // wave's halo pieces k = wave + 8 i (per-lane source offsets at channel group 0;
    // the group moves the buffer's soffset by 128 B)
    // K split (a.ksplit > 1, small batches): item = split * ntiles + tile takes channel
    // groups [cg0, cg1) of its tile and stores the raw partial accumulators;
    // conv_h_finish_kernel sums them and runs the epilogue
    const uint32_t ks = SPLIT ? a.ksplit : 1u, ntiles = a.cls[0].ntiles;
    uint32_t cb = 0, pix0 = 0, bimg = 0, y0 = 0, x0 = 0, hoff[6], cg0 = 0, cg1 = nC;
    auto setup = [&](uint32_t item) {
        uint32_t ln = lane, wv = wave;        // opaque: computed here, not hoisted
        asm volatile("" : "+v"(ln), "+s"(wv));
        uint32_t tile = item;
        if constexpr (SPLIT) {
            const uint32_t split = item / ntiles;
            tile = item - split * ntiles;
            cg0 = split * nC / ks;
            cg1 = (split + 1) * nC / ks;
        }
        cb = tile % nB;
        uint32_t blk = tile / nB;
        const uint32_t bx = blk % nbx;
        blk /= nbx;
        const uint32_t by = blk % nby, b = blk / nby;
        bimg = b;
        y0 = by * 16;
        x0 = bx * 16;
        pix0 = (b * H + y0) * W + x0;
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
    const uint32_t n = lane & 15u, g = lane >> 4;
    // fragment lane bases (bytes within a halo buffer): [column shift dx + 1][lo]
    uint32_t fb0[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int lo = 0; lo < 2; ++lo)
            fb0[d][lo] = (4u * wn * kHaloW + n) * 128u + (((2u * g + lo) ^ halo_swz(n + d)) << 4);
    const uint32_t hs0 = lds_addr(&Hs[0][0]), hs1 = lds_addr(&Hs[1][0]);

    auto fire_w = [&](uint32_t c, uint32_t tap, uint32_t stage) {
        const uint32_t wsoff = __builtin_amdgcn_readfirstlane(
            ((tap * nC + c) * nB + cb) * kStepF4 * 16u + 2 * wave * 1024u);
        set_m0(lds_addr(&As[stage][2 * wave * 64]));
        dma16<0>(uni(rw), lane * 16u, wsoff);
        dma16<1024>(uni(rw), lane * 16u, wsoff);
    };
    uint32_t hsoff = 0;                   // soffset of the group being fetched (c * 128 B)
    auto fire_h = [&](int buf, int i) {
        halo_fire(rx, &Hs[buf][(wave + 8u * i) * 64], hoff[i], hsoff);
    };
    // the current tile's epilogue operands -> Ep (wave w moves piece w; null tensors
    // and the idle lanes read past num_records = zeros)
    auto fire_ep = [&] {
        if (wave >= kEpPieces) return;
        uint32_t lane = tid & 63u;            // opaque: computed here, not hoisted
        asm volatile("" : "+v"(lane));
        const ActEpi &e = a.e;
        const uint32_t OOB = 0x7FFFFFF0u;
        const uint32_t ch = cb * kCT + 4u * (lane & 31u), lo = lane < 32;
        const uint32_t bc = a.B * a.Cout * 4u;
        const float *base;
        uint32_t bytes, off;
        if (wave == 0) {
            base = e.demod; bytes = bc; off = lo ? (bimg * a.Cout + ch) * 4u : OOB;
        } else if (wave == 1) {
            base = e.bias; bytes = a.Cout * 4u; off = lo ? ch * 4u : OOB;
        } else if (wave == 2) {
            base = e.s_next; bytes = e.s_next ? bc : 0u; off = lo ? (bimg * a.Cout + ch) * 4u : OOB;
        } else if (wave == 3 || wave == 4) {
            const uint32_t o = wave == 3 ? (lane >> 5) : 2u;
            const bool ok = wave == 3 || lo;
            if (e.rgb_base) {
                base = e.rgb_base; bytes = 3u * a.Cout * 4u; off = ok ? (o * a.Cout + ch) * 4u : OOB;
            } else {
                base = e.rgb_w; bytes = e.rgb_w ? 3u * bc : 0u;
                off = ok ? ((bimg * 3u + o) * a.Cout + ch) * 4u : OOB;
            }
        } else if (wave == 5) {
            base = e.noise; bytes = e.noise ? a.B * H * W * 4u : 0u;
            off = ((bimg * H + y0 + (lane >> 2)) * W + x0 + 4u * (lane & 3u)) * 4u;
        } else {
            base = e.rgb_s; bytes = e.rgb_base ? bc : 0u; off = lo ? (bimg * a.Cout + ch) * 4u : OOB;
        }
        set_m0(lds_addr(&Ep[wave * 64]));
        dma16<0>(uni(make_rsrc(base, bytes)), off, 0u);
    };

    f4 acc[4][4];

    // fragments of tap T of a channel group whose halo lies at byte hs: A from stage
    // T % 3, B at the tap's offset (dy, dx) = (T / 3 - 1, T % 3 - 1)
    auto read_frags = [&](f4 (&R)[16], auto tapc, uint32_t hs) {
        constexpr int T = decltype(tapc)::value;
        constexpr uint32_t st = T % 3, dyp = T / 3, dxp = T % 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            R[i] = As[st][((4 * wm + i) * 2) * 64 + lane];
            R[4 + i] = As[st][((4 * wm + i) * 2 + 1) * 64 + lane];
        }
        const uint32_t bh = hs + fb0[dxp][0], bl = hs + fb0[dxp][1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t imm = ((j + dyp) * kHaloW + dxp) * 128u;
            R[8 + j] = lds_f4(bh + imm);
            R[12 + j] = lds_f4(bl + imm);
        }
    };
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

    // split term t (0: lo.hi, 1: hi.lo, 2: hi.hi; mfma_rows' order) of row i
    auto mfma_quad = [&](const f4 (&R)[16], int i, int t) {
        const f4 &ra = t == 0 ? R[4 + i] : R[i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = mfma16(ra, t == 1 ? R[12 + j] : R[8 + j], acc[i][j]);
    };

    // prologue of a tile: halo of group 0, weights of steps 0-2 (every LDS buffer is
    // free once all waves passed the previous tile's last barrier)
    auto prologue = [&] {
        hsoff = cg0 * 128u;
#pragma unroll
        for (int i = 0; i < 6; ++i) fire_h(0, i);
        hsoff += 128u;                    // next: group cg0 + 1
        fire_w(cg0, 0, 0);
        fire_w(cg0, 1, 1);
        fire_w(cg0, 2, 2);
    };

    // persistent schedule: this workgroup's share of the ntiles * ks items
    const XcdShare sh = xcd_share(ntiles * ks);
    const uint32_t nwg = sh.stride, tend = sh.end;
    uint32_t tile = sh.first;
    if (tile >= tend) return;    // idle workgroup (whole)
    uint32_t next = tile + nwg;
    bool has_next = next < tend;

    // K-step (c, T): MFMAs of rows 0-1; wait for step (c, T)+1 (in flight may stay only
    // what step (c, T)-1 fired); barrier; fire step +3's weights (into stage T % 3) and,
    // at taps 0-5, halo piece T of group c + 1 (into the buffer group c - 1 used, whose
    // last fragment reads were before the barrier of (c - 1, 8)); read step +1's
    // fragments; MFMAs of rows 2-3.  The tile's second step also fires the epilogue
    // operands (older than everything step 3 waits for); the last one fires the next
    // tile's prologue.
    // P: parity of group c (its halo buffer), compile-time in the unrolled loop
    auto step = [&](uint32_t c, auto tapc, auto parc, const f4 (&R)[16], f4 (&Rn)[16]) {
        constexpr int T = decltype(tapc)::value;
        constexpr int P = decltype(parc)::value;
        const uint32_t s = (c - cg0) * 9 + T, nk = (cg1 - cg0) * 9;
        const bool prev_w = s + 2 < nk;                     // step s-1 fired weights
        const bool prev_h = T != 0 && T - 1 <= 5 && c + 1 < cg1;  // ... and a halo piece
        mfma_rows(R, 0, 2);
        if (prev_w && prev_h) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
        else if (prev_w) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if constexpr (T == 1) {
            if (c == cg0 && !SPLIT) fire_ep();
        }
        // Issue order after the barrier, pinned by scheduling fences (left to itself
        // the compiler clumps all DMAs and reads in front of the MFMAs, and an LDS-DMA
        // issued in such a clump costs the wave several times its price between
        // MFMAs; measured -3.7 % conv time): the next step's 16 fragment reads one per
        // MFMA of row 2 (after the last step they read stale data nobody uses), then
        // the weight pair and the halo piece (and after the last step the next tile's
        // prologue) between the three MFMA quads of row 3.
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (T == 8) read_frags(Rn, std::integral_constant<int, 0>{}, P ? hs0 : hs1);
        else read_frags(Rn, std::integral_constant<int, T + 1>{}, P ? hs1 : hs0);
        mfma_rows(R, 2, 1);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_quad(R, 3, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 3 < nk) {
            constexpr uint32_t T3 = (T + 3) % 9;
            fire_w(c + (T + 3) / 9, T3, T % 3);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_quad(R, 3, 1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (T <= 5) {
            if (c + 1 < cg1) fire_h(1 - P, T);
        }
        if constexpr (T == 8) {
            if (s + 1 == nk && has_next) {
                setup(next);
                prologue();
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_quad(R, 3, 2);
        __builtin_amdgcn_sched_barrier(0);
    };

    setup(tile);
    prologue();
    bool first = true;
    for (;;) {
        const uint32_t ecb = cb, epix0 = pix0, eb = bimg;    // this tile (setup moves on)
        const uint32_t eitem = tile, c1 = cg1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        // everything but step 2's weights has landed (after the first tile: everything,
        // the previous epilogue's stores included); the previous epilogue's LDS reads
        // are done everywhere after the barrier
        if (first) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        f4 R0[16], R1[16];
        read_frags(R0, std::integral_constant<int, 0>{}, hs0);
        // two channel groups per iteration: 18 steps alternate R0 / R1.  (Spelled out: the
        // nine steps of a group behind a lambda, as conv_t_kernel has them, compile to
        // other code.)
        uint32_t c = cg0;
        for (; c + 1 < c1; c += 2) {
            step(c, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 3>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 4>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 5>{}, std::integral_constant<int, 0>{}, R1, R0);
            hsoff += 128u;
            step(c, std::integral_constant<int, 6>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 7>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 8>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c + 1, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, R1, R0);
            step(c + 1, std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, R0, R1);
            step(c + 1, std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}, R1, R0);
            step(c + 1, std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{}, R0, R1);
            step(c + 1, std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{}, R1, R0);
            step(c + 1, std::integral_constant<int, 5>{}, std::integral_constant<int, 1>{}, R0, R1);
            hsoff += 128u;
            step(c + 1, std::integral_constant<int, 6>{}, std::integral_constant<int, 1>{}, R1, R0);
            step(c + 1, std::integral_constant<int, 7>{}, std::integral_constant<int, 1>{}, R0, R1);
            step(c + 1, std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{}, R1, R0);
        }
        if (c < c1) {
            step(c, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 3>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 4>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 5>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 6>{}, std::integral_constant<int, 0>{}, R0, R1);
            step(c, std::integral_constant<int, 7>{}, std::integral_constant<int, 0>{}, R1, R0);
            step(c, std::integral_constant<int, 8>{}, std::integral_constant<int, 0>{}, R0, R1);
        }
        if (SPLIT) {    // raw partials of this split: [item][16 (i, j)][512 threads] f4
            f4 *pp = a.partial + (size_t)eitem * 16 * 512 + tid;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) pp[(i * 4 + j) * 512] = acc[i][j];
        } else {
            conv_h_epilogue(a, acc, Ep, lane, wm, wn, ecb, epix0, eb);
        }
        if (!has_next) break;
        tile = next;
        next = tile + nwg;
        has_next = next < tend;
        first = false;
    }
}

// conv_h_kernel's K-split finish: the ksplit partial tiles summed in split order
// (deterministic; the same K ranges and order as conv_x_kernel's split), then the
// fused epilogue.  A workgroup is a QUARTER tile: the two waves (wm = 0, 1) of one
// n-tile row group wn = blockIdx.y, so the finish of a batch-1 layer spreads over 4x the
// CUs of the conv (64 -> 256 workgroups at 64^2).
__global__ void __launch_bounds__(128) conv_h_finish_kernel(const ConvArgs a) {
    const uint32_t tile = blockIdx.x, wn = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wm = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ntiles = a.cls[0].ntiles;
    const uint32_t tid = (wm + 2u * wn) * 64u + lane;       // conv_h_kernel's thread of it
    const uint32_t nB = a.Cout / kCT, nbx = a.Win / 16, nby = a.Hin / 16;
    const uint32_t cb = tile % nB, blk = tile / nB;
    const uint32_t bx = blk % nbx, by = (blk / nbx) % nby, b = blk / (nbx * nby);
    const uint32_t pix0 = (b * a.Hin + by * 16u) * a.Win + bx * 16u;
    f4 acc[4][4], t[3][16];
    const f4 *pp = a.partial + (size_t)tile * 16 * 512 + tid;
    const size_t sstride = (size_t)ntiles * 16 * 512;
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
    conv_epilogue<true>(a, acc, lane, wm, wn, cb, pix0, a.B * a.Hin * a.Win, a.Hin, a.Win, 0, 0,
                        a.Win, 0, 0);
}

}  // namespace
}  // namespace sdfr

// field_r.h -- field_r_kernel, the split-fp16 field kernel with one wave per SIMD (the ngp
// and FC networks), with its weight ring (RRing, r_dma*), k-step (rstep), activation (r_act)
// and tail helpers.  Instantiated by field_f16x3.hip (render), field_query.hip and
// field_fc_query.hip (point queries); field_grad.hip builds field_g_kernel on rstep.
#pragma once

#include "field_common.h"

namespace sdfr {

typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void xpin(f2v &x) { asm volatile("" : "+v"(x)); }

constexpr int kRValuPerMfma = 5;           // field_r_kernel: VALU slots after each MFMA
constexpr int kRDsPerMfma = 2;             // field_r_kernel: LDS-read slots after each MFMA

// ----------------------------------------------------------------------------
// field_r_kernel: one wave per SIMD on v_mfma_f32_32x32x16_f16.
//
// Design history (round 4, measured, git history): round 3's field_p_kernel put two waves
// on each SIMD (256 VGPRs each) that split every layer's rows and handed each layer's
// input across through LDS (exchange writes, B reads, 2-way bank conflicts); a one-wave
// 16x16x32 variant (field_q_kernel) removed the hand-off and ran at the same speed
// (55 % MFMA busy, 34 % of wave cycles waiting on issue: a 16-cycle MFMA leaves one wave
// two issue slots).  This kernel issues 32x32x16 MFMAs (32 cycles, the vector issue held
// for 8 of them): the same work per FLOP with three times the free issue slots.
// Opaque-register ablations (scripts/build_variants.sh; a plain "reuse the A registers"
// ablation lets hipcc merge identical MFMA chains and is invalid) priced the parts per
// SIMD: the A-fragment LDS reads ~1 % of cycles, the LDS-DMA issue ~8 %, a barrier per
// k-step ~9 % (now one per k-step pair), the colour tail ~13 % (now software pipelined).
//
// Work unit: a workgroup of 4 waves (one per SIMD, 512 VGPRs) over 4 tiles of 16 rays;
// wave w takes tile w, 2 samples of each of its 16 rays per pass: MFMA column
// c = lane & 31 is ray c & 15, sample 2p + (c >> 4); lane half h = lane >> 5.  Output
// tile T (32 rows of a 256-wide layer) is 16 accumulators per lane, register v holding
// row 32 T + (v & 3) + 8 (v >> 2) + 4 h.  Registers 8 s' .. 8 s' + 7 (s' = 0, 1) of a tile,
// activated and split, are the B fragment of k-step 2 T + s' of the next layer (element
// j = row 32 T + 16 s' + 8 (j >> 2) + 4 h + (j & 3)); the packed weights permute K to match
// (xprep_kernel, rperm_k).  Per k-step (16 K) and wave: 8 tiles x 3 split terms = 24
// MFMAs (768 cycles), 16 A ds_read_b128, 4 LDS-DMA pieces of the 16 KB weight slice.
struct RRing {
    f4 *lds;          // weight ring: 4 slots of kRSliceF4
    v4i drsrc;
    uint32_t tid, wave;
    uint32_t ubase;   // ring half of the pass's unit 0 (units per pass may be odd)
    f4 na[3][2];      // the next k-step's groups 0-2 A fragments (hi, lo)
};

// this wave's 4 pieces of slice SLICE -> ring slot `slot` (instruction offsets 0..3 KB
// move the global and the LDS address alike)
template <uint32_t SLICE>
__device__ __forceinline__ void r_dma(const RRing &R, uint32_t slot) {
    const uint32_t sbase = R.wave * 4096u;
    const uint32_t lbase = lds_addr(R.lds) + sbase + slot * (kRSliceF4 * 16u);
    const uint32_t voff = (R.tid & 63u) * 16u;
    uint32_t keep, so;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_add_u32 %1, %5, %6\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %2, %3, %1 offen lds\n\t"
        "buffer_load_dwordx4 %2, %3, %1 offen offset:1024 lds\n\t"
        "buffer_load_dwordx4 %2, %3, %1 offen offset:2048 lds\n\t"
        "buffer_load_dwordx4 %2, %3, %1 offen offset:3072 lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&s"(so)
        : "v"(voff), "s"(R.drsrc), "s"(lbase), "s"(sbase), "i"(SLICE * kRSliceF4 * 16u)
        : "memory", "scc");
}

// Ring units: k-steps (2u, 2u + 1) of a pass, the last k-step alone when a pass has an odd
// count; unit U (counted over all passes) holds the ring half U & 1 (slots 2 (U & 1) +
// 0, 1).  One barrier per unit, in its last k-step: behind it unit U + 2 is DMA'd into
// unit U's half.
template <class Net>
__device__ __forceinline__ uint32_t r_slot(const RRing &R, int ks) {
    return 2u * ((R.ubase + (uint32_t)(ks >> 1)) & 1u) + (uint32_t)(ks & 1);
}

// One LDS-DMA piece: this wave's 1 KB at offset K KB of its 4 KB share of slice SLICE
template <uint32_t SLICE, uint32_t K>
__device__ __forceinline__ void r_dma1(const RRing &R, uint32_t slot) {
    const uint32_t sbase = R.wave * 4096u;
    const uint32_t lbase = lds_addr(R.lds) + sbase + slot * (kRSliceF4 * 16u);
    const uint32_t voff = (R.tid & 63u) * 16u;
    uint32_t so;
    // (M0 is not restored: no compiler-generated code in field_r_kernel reads M0 --
    // checked in the ISA, as for the conv kernels' set_m0)
    asm volatile(
        "s_mov_b32 m0, %3\n\ts_add_u32 %0, %4, %5\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %0 offen offset:%6 lds"
        : "=&s"(so)
        : "v"(voff), "s"(R.drsrc), "s"(lbase), "s"(sbase), "i"(SLICE * kRSliceF4 * 16u),
          "i"(K * 1024u)
        : "memory", "scc");
}

// Piece P (0..7: slice P >> 2, 1 KB part P & 3) of in-pass unit V (V >= units per pass:
// the next pass's unit V - UPP) into ring half `half`
template <class Net, int V, int P>
__device__ __forceinline__ void r_dma_piece(const RRing &R, uint32_t half) {
    constexpr int NS = RNet<Net>::kSteps, UPP = (NS + 1) / 2;
    constexpr int S = 2 * (V % UPP) + (P >> 2);
    if constexpr (S < NS) r_dma1<(uint32_t)S, (uint32_t)(P & 3)>(R, 2u * half + (uint32_t)(P >> 2));
}

// One k-step of one wave: 8 output tiles x 3 split terms = 24 MFMAs in 8 groups of one
// tile.  Group gi's A fragments (hi, lo) were read during group gi - 3 (groups 0-2: by the
// previous k-step, R.na).  In a unit's last k-step the barrier (this wave's DMA of the next
// unit landed, its A reads of this unit done) sits ahead of group 5; behind it the unit
// after next is DMA'd into this unit's half, one 1 KB piece per MFMA group (three in
// groups 5-7, five in the next k-step's groups 0-4), and the next k-step's groups 0-2 A
// fragments are read.  side(gi) runs between group gi's MFMAs.
template <class Net, int KS, bool ZC, class Side>
__device__ __forceinline__ void rstep(RRing &R, f16v (&acc)[8], const f4 (&bf)[2], Side &&side) {
    constexpr int NS = RNet<Net>::kSteps;
    constexpr bool kBar = (KS & 1) || KS == NS - 1;         // the unit's last k-step
    constexpr int U = KS >> 1;
    const uint32_t lane = R.tid & 63u;
    const f4 *A = R.lds + r_slot<Net>(R, KS) * kRSliceF4 + lane;
    const f4 *An = R.lds + r_slot<Net>(R, KS + 1) * kRSliceF4 + lane;
    const uint32_t half = (R.ubase + (uint32_t)U) & 1u;     // = the half of unit U + 2
    f4 a[8][2];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        a[g][0] = R.na[g][0];
        a[g][1] = R.na[g][1];
    }
    sfor<0, 8>([&](auto GI) {
        constexpr int gi = decltype(GI)::value;
        if constexpr (kBar && gi == 5) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        // the unit's barrier releases unit U + 2's pieces 0-2 here (groups 5-7) and
        // 3-7 in the first k-step of unit U + 1 (groups 0-4): at KS (a unit's first
        // k-step) those are unit U + 1's (behind the previous k-step's barrier; in a
        // workgroup's first pass they repeat the prologue's bytes)
        // (a pass with an odd k-step count ends in a one-k-step unit whose barrier
        // would wait on pieces issued just before it: the unit before it issues all
        // eight of unit U + 2's pieces behind its own barrier, 3 + 3 + 2)
        constexpr bool kOdd = (NS & 1) != 0;
        constexpr bool kLastSingle = kOdd && KS == NS - 1;
        constexpr bool kBeforeSingle = kOdd && KS == NS - 2;
        if constexpr (kBar && gi >= 5) {
            if constexpr (kBeforeSingle) {
                sfor<3 * (gi - 5), (3 * (gi - 4) < 8 ? 3 * (gi - 4) : 8)>([&](auto PP) {
                    r_dma_piece<Net, U + 2, decltype(PP)::value>(R, half);
                });
            } else {
                r_dma_piece<Net, U + 2, gi - 5>(R, half);
            }
        }
        if constexpr ((KS & 1) == 0 && !kLastSingle && gi < 5)
            r_dma_piece<Net, U + 1, gi + 3>(R, (R.ubase + (uint32_t)U + 1u) & 1u);
        if constexpr (gi + 3 < 8) {
            a[gi + 3][0] = A[(gi + 3) * 128];
            a[gi + 3][1] = A[(gi + 3) * 128 + 64];
        } else if constexpr (KS + 1 < NS) {
            // (the next pass's first fragments are read after the pass tail, r_na)
            R.na[gi - 5][0] = An[(gi - 5) * 128];
            R.na[gi - 5][1] = An[(gi - 5) * 128 + 64];
        }
        side(GI);
        constexpr f16v kZ = {};
        // W_lo x_hi, W_hi x_lo, W_hi x_hi
        acc[gi] = mfma32(a[gi][1], bf[0], ZC ? kZ : acc[gi]);
        acc[gi] = mfma32(a[gi][0], bf[1], acc[gi]);
        acc[gi] = mfma32(a[gi][0], bf[0], acc[gi]);
        asm volatile("" ::"v"(a[gi][0]), "v"(a[gi][1]));
        sfor<0, 3>([&](auto I) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, kRDsPerMfma, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, kRValuPerMfma, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
    });
}

// groups 0-2 A fragments of the k-step in ring slot `slot` (landed: behind its barrier)
__device__ __forceinline__ void r_na(RRing &R, uint32_t slot) {
    const f4 *A = R.lds + slot * kRSliceF4 + (R.tid & 63u);
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        R.na[g][0] = A[g * 128];
        R.na[g][1] = A[g * 128 + 64];
    }
}

// FiLM activation of registers 8 s' .. 8 s' + 7 of output tile T into v[8] (element j =
// register 8 s' + j): film rows 32 T + 16 s' + 4 h + (0..3) (gm0, bt0, w0) and + 8 (gm1, ...);
// SIN false: ReLU(fma(1/su, z, b)) (FcNet)
template <int MODE, bool SIN = true>
__device__ __forceinline__ void r_act(const f16v &z, int sp, const f4 &gm0, const f4 &bt0,
                                      const f4 &w0, const f4 &gm1, const f4 &bt1, const f4 &w1,
                                      float &sdfp, int es, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float zz = z[8 * sp + j];
        const float g = j < 4 ? gm0[j & 3] : gm1[j & 3], b = j < 4 ? bt0[j & 3] : bt1[j & 3];
        if constexpr (!SIN) v[j] = fmaxf(__fmaf_rn(g, zz, b), 0.0f);
        else if constexpr (MODE == 0) v[j] = sin_rev(__fmaf_rn(g, __builtin_ldexpf(zz, -es), b));
        else v[j] = sin_rev(__fmaf_rn(g, zz, b));
        if constexpr (MODE == 2) sdfp = __fmaf_rn(v[j], j < 4 ? w0[j & 3] : w1[j & 3], sdfp);
    }
}

// v_permlane16_swap of (pa, pb) between the two 16-lane rows of each pair: the even
// row gets pa(even) + pa(odd), the odd row pb(even) + pb(odd).  The results pass through
// an empty asm: on float values bit-cast to the builtin's operands, hipcc (ROCm 7.2)
// returned the first result twice (checked on a probe kernel's ISA).
__device__ __forceinline__ float row_pair_sum(float pa, float pb) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, pa),
                                                     __builtin_bit_cast(uint32_t, pb), false, false);
    uint32_t r0 = sw[0], r1 = sw[1];
    asm volatile("" : "+v"(r0), "+v"(r1));
    return __fadd_rn(__builtin_bit_cast(float, r0), __builtin_bit_cast(float, r1));
}

// Round-to-nearest hi / lo fp16 split of channels c .. c + 3 of an 8-channel group held
// by lane half h (lanes l, l ^ 32 hold channels 0-3 and 4-7) into split-NHWC
// ([pixel][C / 8][hi 8, lo 8]; idx8 = NHWC element index of the group's channel 0): one
// v_permlane32_swap per dword gives lane h = 0 both hi halves and lane h = 1 both lo
// halves, so each lane issues one 16-B store.  Both lanes of a pair must execute it.
// (integer operands, results pinned as for row_pair_sum)
typedef _Float16 h4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_split8_pair32(_Float16 *ys, size_t idx8, f4 v, uint32_t h) {
    // v pinned: hipcc otherwise folds the caller's fp32 product into the fp16 conversion
    // (v_fma_mixlo_f16: one rounding instead of modulate_nhwc_kernel's two -- a tie of
    // the fp32 product then rounds the other way)
    asm volatile("" : "+v"(v));
    h4f hi, lo;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        hi[r] = (_Float16)v[r];
        lo[r] = (_Float16)(v[r] - (float)hi[r]);
    }
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    const u2 hd = __builtin_bit_cast(u2, hi), ld = __builtin_bit_cast(u2, lo);
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const auto sw = __builtin_amdgcn_permlane32_swap(hd[k], ld[k], false, false);
        uint32_t r0 = sw[0], r1 = sw[1];
        asm volatile("" : "+v"(r0), "+v"(r1));
        q[k] = r0;          // h = 0: own hi / h = 1: partner's lo
        q[2 + k] = r1;      // h = 0: partner's hi / h = 1: own lo
    }
    *reinterpret_cast<f4 *>(ys + 2 * idx8 + (h ? 8 : 0)) = __builtin_bit_cast(f4, q);
}

// Element e of FCGenerator.transform_points (sdf_model.py:1628-1640) of ph = p / 2:
// e = 6 i + r, sin (r < 3) or cos (r >= 3) of (2^i pi) ph[r mod 3], with the reference's
// fp32 argument RN(RN32(2^i pi) ph) (a Python float times an fp32 tensor).  The sine of
// that fp32 argument: reduced to revolutions in fp64 (exact product, fraction to 2^-40),
// then v_sin_f32 (< 1e-6 absolute, tests/test_gpu_encoders.py).
__device__ __forceinline__ float posenc_val(const float (&ph)[3], uint32_t e) {
    const uint32_t i = e / 6u, r = e - 6u * i;
    const uint32_t c = r < 3u ? r : r - 3u;
    const float pc = c == 0u ? ph[0] : (c == 1u ? ph[1] : ph[2]);
    const float arg = __fmul_rn(__builtin_ldexpf(3.14159265358979323846f, (int)i), pc);
    double u = (double)arg * 0.15915494309189533577;     // 1 / (2 pi)
    if (r >= 3u) u += 0.25;                               // cos x = sin(x + pi / 2)
    u -= floor(u);
    return sin_rev((float)u);
}

template <class Net>
__global__ void __launch_bounds__(kRThreads, 1) field_r_kernel(const XFieldArgs a) {
    constexpr int NF = Net::kFilmN;
    constexpr int KV = RNet<Net>::kViews;
    constexpr int KL0 = RNet<Net>::kL0;
    constexpr int NS = RNet<Net>::kSteps;
    constexpr int NL = Net::kLayers;
    constexpr bool Q = Net::kQuery;                         // point query: no ray, no compositing
    __shared__ f4 ring_lds[4 * kRSliceF4];                  // 64 KB weight ring
    __shared__ f4 facc_lds[kRWaves][16][64];                // 64 KB: [wave][f4 of 64 features][lane]
    __shared__ float film_lds[NF * 2 * kW];                 // the workgroup's face
    __shared__ float cst[4 * kW];                           // sigma_w, rgb_w[3]
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t c = lane & 31u, h = lane >> 5, r16 = c & 15u;
    const bool odd = c >= 16u;                              // sample 2p + 1 of the pass
    const GeomArgs &G = a.g;

    const uint32_t wg_per_face = (G.tiles_per_face + kRTiles - 1) / kRTiles;
    const uint32_t seg = blockIdx.x % a.nseg, blk = blockIdx.x / a.nseg;
    const uint32_t b = blk / wg_per_face;
    const float beta_s = a.with_sdf ? a.sigmoid_beta[0] : 1.0f;
    {
        const f4 *src = reinterpret_cast<const f4 *>(a.film + (size_t)b * NF * 2 * kW);
        f4 *dst = reinterpret_cast<f4 *>(film_lds);
        for (uint32_t i = tid; i < NF * 2 * kW / 4; i += kRThreads) dst[i] = src[i];
    }
    RRing R;
    R.lds = ring_lds;
    R.tid = tid;
    R.wave = wave;
    R.ubase = 0;
    R.drsrc = make_rsrc(a.packed, Net::kSlices * kXSliceF4 * sizeof(f4));
    for (uint32_t i = tid; i < 4 * kW; i += kRThreads)
        cst[i] = i < kW ? a.sigma_w[i] : a.rgb_w[i - kW];
    // prologue: units 0, 1 (slices 0-3) -> slots 0-3 (unit U's barrier issues unit U + 2)
    r_dma<0>(R, 0);
    r_dma<1>(R, 1);
    r_dma<2>(R, 2);
    r_dma<3>(R, 3);
    f4 *facc = &facc_lds[wave][0][lane];
    if constexpr (!Q) {
#pragma unroll
        for (int t = 0; t < 16; ++t) facc[t * 64] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const float *sig_w = cst, *rgb_w = cst + kW;
    auto fg = [&](int f) { return (const float *)film_lds + f * 2 * kW; };
    auto fb = [&](int f) { return (const float *)film_lds + f * 2 * kW + kW; };
    const float sig_b = a.sigma_b[0];
    const float rgb_b0 = a.rgb_b[0], rgb_b1 = a.rgb_b[1], rgb_b2 = a.rgb_b[2];
    const uint32_t npass = (G.N + kRSamples - 1) / kRSamples;
    const uint32_t pps = (npass + a.nseg - 1) / a.nseg;
    const uint32_t p_begin = seg * pps, p_end = min(npass, p_begin + pps);

    uint32_t tile_local = (blk % wg_per_face) * kRTiles + wave;
    const bool tile_ok = tile_local < G.tiles_per_face;
    if (!tile_ok) tile_local = G.tiles_per_face - 1;
    const uint32_t tile = b * G.tiles_per_face + tile_local;
    uint32_t ray_local = tile_local * kTileRays + r16;
    const bool ray_ok = tile_ok && ray_local < G.H * G.W;
    if (ray_local >= G.H * G.W) ray_local = G.H * G.W - 1;
    const uint32_t py = ray_local / G.W, px = ray_local % G.W;
    const uint32_t ray_index = (b * G.H + py) * G.W + px;

    Ray ray;
    if constexpr (!Q)
        make_ray(G.cam + (size_t)b * 12, G.focal[b], G.pix_x[px], G.pix_y[py], G.half_res, ray);
    const float nr = Q ? 0.0f : G.near_[b], fr = Q ? 0.0f : G.far_[b];
    const float span = __fsub_rn(fr, nr);
    const float dnorm = Q ? 0.0f : norm3_torch(ray.d[0], ray.d[1], ray.d[2]);
    constexpr int NVX = Net::kViewSteps - 16;
    f4 vx[NVX][2];                                          // the views layer's k-steps 16 (, 17)
    {
        float ux, uy, uz;
        if constexpr (Q) {
            // the group's direction as the network sees it (unit length already):
            // dirs [B,R,3] in G.cam, ray_index = b R + group (H = 1, W = R)
            const float *dv = G.cam + (size_t)ray_index * 3;
            ux = dv[0];
            uy = dv[1];
            uz = dv[2];
        } else {
            const float v0 = G.static_viewdirs ? ray.dir[0] : ray.d[0];
            const float v1 = G.static_viewdirs ? ray.dir[1] : ray.d[1];
            const float v2 = G.static_viewdirs ? ray.dir[2] : ray.d[2];
            const float vn = norm3_torch(v0, v1, v2);
            ux = __fdiv_rn(v0, vn), uy = __fdiv_rn(v1, vn), uz = __fdiv_rn(v2, vn);
        }
        float v[8];
        if constexpr (Net::kPosEnc) {
            // transform_points(views, True) (sdf_model.py:1628-1640): p / 2, 4 frequencies
            const float ph[3] = {__fmul_rn(ux, 0.5f), __fmul_rn(uy, 0.5f), __fmul_rn(uz, 0.5f)};
#pragma unroll
            for (int st = 1; st < NVX; ++st) {
                float w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t e = 16 * st + 8 * h + j;
                    w[j] = e < Net::kPosViews ? posenc_val(ph, e) : 0.0f;
                }
                split8(w, vx[st][0], vx[st][1]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = posenc_val(ph, 8 * h + j);
        } else if constexpr (Net::kSiren) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = 0.0f;
            if (h == 0) {
                v[0] = ux;
                v[1] = uy;
                v[2] = uz;
            }
        } else {
            const f4 qa = sh_quad(ux, uy, uz, 2 * h), qb = sh_quad(ux, uy, uz, 2 * h + 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = qa[r];
                v[4 + r] = qb[r];
            }
        }
        split8(v, vx[0][0], vx[0][1]);
    }
    float T = 1.0f, wsum = 0.0f, racc0 = 0.0f, racc1 = 0.0f, racc2 = 0.0f;
    float xacc0 = 0.0f, xacc1 = 0.0f, xacc2 = 0.0f, w_last = 0.0f;
    const size_t tile_sid = (size_t)(tile * G.N) * kTileRays + r16;
    const __amdgpu_buffer_rsrc_t enc_r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.enc), (short)0, Net::kGrid ? (int)(16u * G.S_total * 8u) : 0, 0x00020000);
    float2 en[2][4];                                        // [layer-0 k-step][level pair]
    float pin[3];                                           // FcNet: normalised point / 2
    auto load_inputs = [&](uint32_t p) {
        uint32_t s = kRSamples * p + (odd ? 1u : 0u);
        if (s >= G.N) s = G.N - 1;
        if constexpr (Net::kPosEnc && Q) {
            // the caller's point (network coordinates): points [B,R,N,3] in a.enc; padding
            // groups and samples read a clamped, valid one
            const float *pv = a.enc + ((size_t)ray_index * G.N + s) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) pin[k] = __fmul_rn(pv[k], 0.5f);
        } else if constexpr (Net::kPosEnc) {
            const float z = sample_z(G.sc, nr, fr, ray_index, s);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float pp = __fadd_rn(ray.o[k], __fmul_rn(ray.d[k], z));
                pin[k] = __fmul_rn(G.z_normalize ? __fdiv_rn(__fmul_rn(pp, 2.0f), span) : pp, 0.5f);
            }
        } else if constexpr (Net::kSiren) {
            const float z = sample_z(G.sc, nr, fr, ray_index, s);
            float np_[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float pp = __fadd_rn(ray.o[k], __fmul_rn(ray.d[k], z));
                np_[k] = G.z_normalize ? __fdiv_rn(__fmul_rn(pp, 2.0f), span) : pp;
            }
            const bool h0 = h == 0;
            en[0][0] = make_float2(h0 ? np_[0] : 0.0f, h0 ? np_[1] : 0.0f);
            en[0][1] = make_float2(h0 ? np_[2] : 0.0f, 0.0f);
            en[0][2] = en[0][3] = make_float2(0.0f, 0.0f);
        } else {
            // buffer loads: one 32-bit lane offset (level 4 h, sample), the level step as a
            // wave-uniform offset (8 hoisted 64-bit addresses otherwise: VGPR pressure)
            const uint32_t voff = ((uint32_t)(tile_sid + (size_t)s * kTileRays) + 4 * h * G.S_total) * 8u;
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // (index the builtin's vector directly: a bit_cast of it to another vector
                    // type made hipcc load one dword and use it twice, ROCm 7.2)
                    const auto v = __builtin_amdgcn_raw_buffer_load_b64(
                        enc_r, (int)voff, (int)((8 * st + k) * G.S_total * 8u), 0);
                    const uint32_t vx0 = v[0], vy0 = v[1];
                    en[st][k] = make_float2(__builtin_bit_cast(float, vx0), __builtin_bit_cast(float, vy0));
                }
        }
    };
    load_inputs(p_begin);

    for (uint32_t p = p_begin; p < p_end; ++p) {
        R.ubase = __builtin_amdgcn_readfirstlane(((p - p_begin) * (uint32_t)((NS + 1) / 2)) & 1u);
        r_na(R, r_slot<Net>(R, 0));
        f16v X[8], Y[8];
        f4 bf[2], E[KL0][2];                               // B fragments: current, layer 0's
        int es = 0;
        if constexpr (Net::kPosEnc) {
            // transform_points(p) (sdf_model.py:1628-1640): 10 frequencies x (sin, cos) of
            // the 3 coordinates; this lane half's 8 of each k-step's 16 (zero past 60)
#pragma unroll
            for (int st = 0; st < KL0; ++st) {
                float w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t e = 16 * st + 8 * h + j;
                    w[j] = e < Net::kPosIn ? posenc_val(pin, e) : 0.0f;
                }
                split8(w, E[st][0], E[st][1]);
            }
        } else {
            float v[16];
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[8 * st + 2 * k] = en[st][k].x;
                    v[8 * st + 2 * k + 1] = en[st][k].y;
                }
            if constexpr (Net::kGrid) {
                // the sample's 32 features over both lane halves -> 2^es into [0.5, 1)
                float m = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j) m = fmaxf(m, fabsf(v[j]));
                m = fmaxf(m, __shfl_xor(m, 32));
                if (m > 0.0f && m < 3.0e38f) {
                    const int ex = __builtin_amdgcn_frexp_expf(m);
                    es = ex < -100 ? 100 : -ex;
#pragma unroll
                    for (int j = 0; j < 16; ++j) v[j] = __builtin_ldexpf(v[j], es);
                }
            }
            float u0[8], u1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                u0[j] = v[j];
                u1[j] = v[8 + j];
            }
            split8(u0, E[0][0], E[0][1]);
            if constexpr (KL0 > 1) split8(u1, E[KL0 - 1][0], E[KL0 - 1][1]);
        }
        float sdfp = 0.0f;
        f4 bn[2];
        struct ActState {
            f4 gm0, bt0, w0, gm1, bt1, w1;
            float v[8];
        };
        ActState as;
        // activation of chunk q (registers 8 (q & 1) .. + 7 of tile q >> 1) of layer l's
        // output o into bn: film vectors read beside group G0, activated beside G0 + 1,
        // split beside G0 + 2
        auto act_side = [&](auto L, f16v (&o)[8], int q, auto GI, auto G0) {
            constexpr int l = decltype(L)::value;
            constexpr int gi = decltype(GI)::value, g0 = decltype(G0)::value;
            constexpr int MODE = (l == 0 && Net::kGrid) ? 0 : (l == NL - 2 ? 2 : 1);
            const int f = Net::film_layer(l);
            const int r0 = 32 * (q >> 1) + 16 * (q & 1) + 4 * (int)h;
            if constexpr (gi == g0) {
                as.gm0 = *reinterpret_cast<const f4 *>(fg(f) + r0);
                as.gm1 = *reinterpret_cast<const f4 *>(fg(f) + r0 + 8);
                as.bt0 = *reinterpret_cast<const f4 *>(fb(f) + r0);
                as.bt1 = *reinterpret_cast<const f4 *>(fb(f) + r0 + 8);
                if constexpr (MODE == 2) {
                    as.w0 = *reinterpret_cast<const f4 *>(sig_w + r0);
                    as.w1 = *reinterpret_cast<const f4 *>(sig_w + r0 + 8);
                }
            } else if constexpr (gi == g0 + 1) {
                r_act<MODE, Net::kSinAct>(o[q >> 1], q & 1, as.gm0, as.bt0, as.w0, as.gm1, as.bt1, as.w1, sdfp, es,
                            as.v);
            } else if constexpr (gi == g0 + 2) {
                split8(as.v, bn[0], bn[1]);
            }
        };
        // layer 0: K = 32 (ngp, 2 k-steps), 3 (siren, 1) or 60 (fc, 4); chunk 0 of its
        // output (tile 0 registers 0-7, final after group 0 of the last layer-0 k-step)
        // from group 1 on
        sfor<0, KL0>([&](auto J) {
            constexpr int j = decltype(J)::value;
            bf[0] = E[j][0];
            bf[1] = E[j][1];
            rstep<Net, j, j == 0>(R, X, bf, [&](auto GI) {
                if constexpr (j == KL0 - 1)
                    act_side(std::integral_constant<int, 0>{}, X, 0, GI, std::integral_constant<int, 2>{});
            });
        });
        // hidden layers 1 .. kHidden: 16 k-steps each (in -> out alternate X / Y)
        auto dense = [&](auto L, f16v (&in)[8], f16v (&out)[8]) {
            constexpr int l = decltype(L)::value;
            sfor<0, 16>([&](auto J) {
                constexpr int j = decltype(J)::value;
                constexpr int KS = KL0 + 16 * (l - 1) + j;
                bf[0] = bn[0];
                bf[1] = bn[1];
                rstep<Net, KS, j == 0>(R, out, bf, [&](auto GI) {
                    if constexpr (j < 15)
                        act_side(std::integral_constant<int, l - 1>{}, in, j + 1, GI,
                                 std::integral_constant<int, 0>{});
                    else
                        act_side(std::integral_constant<int, l>{}, out, 0, GI,
                                 std::integral_constant<int, 2>{});
                });
            });
        };
        sfor<1, Net::kHidden + 1>([&](auto L) {
            constexpr int l = decltype(L)::value;
            if constexpr (l & 1) dense(L, X, Y);
            else dense(L, Y, X);
        });
        constexpr bool kInX = (Net::kHidden & 1) == 0;
        f16v (&vin)[8] = kInX ? X : Y;
        f16v (&vout)[8] = kInX ? Y : X;
        const uint32_t s_own = kRSamples * p + (odd ? 1u : 0u);
        const bool s_ok = s_own < G.N;
        const uint32_t sc_ = s_ok ? s_own : G.N - 1;
        float z = 0.0f, dist = 0.0f, al = 0.0f, sdf_c = 0.0f, w_own = 0.0f;
        float wj[2] = {0.0f, 0.0f};
        sfor<0, Net::kViewSteps>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr int KS = KV + j;
            bf[0] = bn[0];
            bf[1] = bn[1];
            if constexpr (j == 14 && Net::kGrid && !Q) {
                const float2 v = a.zd[tile_sid + (size_t)sc_ * kTileRays];
                z = v.x;
                dist = v.y;
            }
            if constexpr (j == 16) {
                if (p + 1 < p_end) load_inputs(p + 1);
            }
            rstep<Net, KS, j == 0>(R, vout, bf, [&](auto GI) {
                constexpr int gi = decltype(GI)::value;
                if constexpr (j < 15) {
                    act_side(std::integral_constant<int, NL - 2>{}, vin, j + 1, GI,
                             std::integral_constant<int, 0>{});
                } else if constexpr (j == 15 && gi == 0) {
                    bn[0] = vx[0][0];                       // k-step 16's B: the direction
                    bn[1] = vx[0][1];
                    sdf_c = __fadd_rn(__fadd_rn(sdfp, __shfl_xor(sdfp, 32)), sig_b);
                } else if constexpr (j == 16 && gi == 0 && NVX > 1) {
                    bn[0] = vx[NVX - 1][0];                 // fc: k-step 17's B
                    bn[1] = vx[NVX - 1][1];
                } else if constexpr (j == 15 && gi == 1 && !Q) {
                    if constexpr (!Net::kGrid) {
                        z = sample_z(G.sc, nr, fr, ray_index, sc_);
                        dist = (sc_ + 1 < G.N)
                                   ? __fmul_rn(__fsub_rn(sample_z(G.sc, nr, fr, ray_index, sc_ + 1), z), dnorm)
                                   : __fmul_rn(1e10f, dnorm);
                    }
                    float alpha;
                    if (a.with_sdf) {
                        const float sig = __fdiv_rn(sigmoidf_(__fdiv_rn(-sdf_c, beta_s)), beta_s);
                        alpha = 1.0f - expf(-sig * dist);
                    } else {
                        float raw = sdf_c;
                        if (a.sigma_noise) raw += a.sigma_noise[(size_t)ray_index * G.N + sc_];
                        const float sp = raw > 20.0f ? raw : log1pf(expf(raw));
                        alpha = 1.0f - expf(-sp * dist);
                    }
                    al = s_ok ? alpha : 0.0f;
                } else if constexpr (j == 16 && gi == 1 && !Q) {
                    // the pass's two compositing weights, identically in both lanes of a ray
                    const float ao = __shfl_xor(al, 16);
                    const float aj[2] = {odd ? ao : al, odd ? al : ao};
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const uint32_t s = kRSamples * p + k;
                        if (s < G.N) {
                            float w = aj[k] * T;
                            if (a.force_background && s + 1 == G.N) w = 1.0f - wsum;
                            T = T * ((1.0f - aj[k]) + 1e-10f);
                            wsum += w;
                            wj[k] = w;
                        }
                    }
                    w_own = odd ? wj[1] : wj[0];
                }
            });
        });
        // colour features f = sin(gamma_v x + beta_v), rgb dot products, and the ray's
        // feature sums: w f of the two samples added across the lane rows by
        // v_permlane16_swap (a tile-0..3 value to the even row, its tile-4..7 partner to
        // the odd row), each row accumulating its half of the features
        const float *f3g = fg(NF - 1), *f3b = fb(NF - 1);
        // rgb dot products in 4 independent chains per channel (one per row r of a 4-row
        // group), added at the end: no 128-long serial fma chain for the scheduler to wait on.
        // The tail has no MFMA beside it (the issue-bound stretch of a pass), so it runs on
        // packed fp32 (v_pk_fma_f32 / v_pk_mul_f32: two rows' worth of the same element-wise
        // IEEE ops per instruction, results bit-identical to the scalar ops): Pk[o][rp] holds
        // the chains of rows 2 rp, 2 rp + 1
        f2v Pk[3][2] = {};
        // 16 steps (tile t and its permlane partner t + 4, 4-row group bq), software
        // pipelined: the next step's film / rgb vectors and feature partials are read
        // (LDS) while this step's values are computed
        struct TailIn {
            f4 gm[2], bt[2], w0[2], w1[2], w2[2], fa;
        };
        auto tail_load = [&](int it, TailIn &T) {
            const int t = it >> 2, bq = it & 3;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r0 = 32 * (t + 4 * u) + 8 * bq + 4 * (int)h;
                T.gm[u] = *reinterpret_cast<const f4 *>(f3g + r0);
                T.bt[u] = *reinterpret_cast<const f4 *>(f3b + r0);
                T.w0[u] = *reinterpret_cast<const f4 *>(rgb_w + r0);
                T.w1[u] = *reinterpret_cast<const f4 *>(rgb_w + kW + r0);
                T.w2[u] = *reinterpret_cast<const f4 *>(rgb_w + 2 * kW + r0);
            }
            if constexpr (!Q) T.fa = facc[(4 * t + bq) * 64];
        };
        TailIn tin[2];
        tail_load(0, tin[0]);
        sfor<0, 16>([&](auto IT) {
            constexpr int it = decltype(IT)::value, t = it >> 2, bq = it & 3;
            TailIn &T = tin[it & 1];
            if constexpr (it + 1 < 16) tail_load(it + 1, tin[(it + 1) & 1]);
            float fp[2][4];
            // rows (2 rp, 2 rp + 1) of each tile as one f2v
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int rp = 0; rp < 2; ++rp) {
                    float fs[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int r = 2 * rp + h;
                        const float y = __fmaf_rn(T.gm[u][r], vout[t + 4 * u][4 * bq + r], T.bt[u][r]);
                        fs[h] = Net::kSinAct ? sin_rev(y) : y;
                    }
                    const f2v fv = {fs[0], fs[1]};
                    const f2v w0 = {T.w0[u][2 * rp], T.w0[u][2 * rp + 1]};
                    const f2v w1 = {T.w1[u][2 * rp], T.w1[u][2 * rp + 1]};
                    const f2v w2 = {T.w2[u][2 * rp], T.w2[u][2 * rp + 1]};
                    Pk[0][rp] = __builtin_elementwise_fma(fv, w0, Pk[0][rp]);
                    Pk[1][rp] = __builtin_elementwise_fma(fv, w1, Pk[1][rp]);
                    Pk[2][rp] = __builtin_elementwise_fma(fv, w2, Pk[2][rp]);
                    fp[u][2 * rp] = fv.x;
                    fp[u][2 * rp + 1] = fv.y;
                }
            // (accumulated whether or not the call wants features: no branch here)
            if constexpr (!Q) {
                f4 acc4 = T.fa;
                const f2v wo = {w_own, w_own};
#pragma unroll
                for (int rp = 0; rp < 2; ++rp) {
                    const f2v pa = wo * f2v{fp[0][2 * rp], fp[0][2 * rp + 1]};
                    const f2v pb = wo * f2v{fp[1][2 * rp], fp[1][2 * rp + 1]};
                    acc4[2 * rp] = __fadd_rn(acc4[2 * rp], row_pair_sum(pa.x, pb.x));
                    acc4[2 * rp + 1] = __fadd_rn(acc4[2 * rp + 1], row_pair_sum(pa.y, pb.y));
                }
                facc[(4 * t + bq) * 64] = acc4;
            }
            // the dot-product partials are materialised here (IR sinking otherwise defers
            // all 384 fmas past the loop and keeps every colour feature live: spills)
#pragma unroll
            for (int o = 0; o < 3; ++o)
#pragma unroll
                for (int rp = 0; rp < 2; ++rp) xpin(Pk[o][rp]);
            __builtin_amdgcn_sched_barrier(0);     // one step of look-ahead (VGPRs)
        });
        float P0 = __fadd_rn(__fadd_rn(Pk[0][0].x, Pk[0][0].y), __fadd_rn(Pk[0][1].x, Pk[0][1].y));
        float P1 = __fadd_rn(__fadd_rn(Pk[1][0].x, Pk[1][0].y), __fadd_rn(Pk[1][1].x, Pk[1][1].y));
        float P2 = __fadd_rn(__fadd_rn(Pk[2][0].x, Pk[2][0].y), __fadd_rn(Pk[2][1].x, Pk[2][1].y));
        if (a.sdf && ray_ok && h == 0 && s_ok) a.sdf[(size_t)ray_index * G.N + s_own] = sdf_c;
        {
            P0 = __fadd_rn(P0, __shfl_xor(P0, 32));
            P1 = __fadd_rn(P1, __shfl_xor(P1, 32));
            P2 = __fadd_rn(P2, __shfl_xor(P2, 32));
            if constexpr (Q) {
                // the sample's own colour [B,R,N,3] (the render composites these values)
                if (a.rgb && ray_ok && h == 0 && s_ok) {
                    float *o = a.rgb + ((size_t)ray_index * G.N + s_own) * 3;
                    o[0] = sigmoidf_(__fadd_rn(P0, rgb_b0));
                    o[1] = sigmoidf_(__fadd_rn(P1, rgb_b1));
                    o[2] = sigmoidf_(__fadd_rn(P2, rgb_b2));
                }
                continue;
            }
            racc0 = __fmaf_rn(w_own, sigmoidf_(__fadd_rn(P0, rgb_b0)), racc0);
            racc1 = __fmaf_rn(w_own, sigmoidf_(__fadd_rn(P1, rgb_b1)), racc1);
            racc2 = __fmaf_rn(w_own, sigmoidf_(__fadd_rn(P2, rgb_b2)), racc2);
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (kRSamples * p + k < G.N) w_last = wj[k];
            if (a.xyz) {
                xacc0 = __fmaf_rn(w_own, __fadd_rn(ray.o[0], __fmul_rn(ray.d[0], z)), xacc0);
                xacc1 = __fmaf_rn(w_own, __fadd_rn(ray.o[1], __fmul_rn(ray.d[1], z)), xacc1);
                xacc2 = __fmaf_rn(w_own, __fadd_rn(ray.o[2], __fmul_rn(ray.d[2], z)), xacc2);
            }
        }
    }
    // the ring runs ahead across passes: no LDS-DMA may land after the workgroup ends
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (Q) return;                                // per-sample stores only
    // the two lanes of a ray (samples 2p, 2p + 1) add their partials
    racc0 = __fadd_rn(racc0, __shfl_xor(racc0, 16));
    racc1 = __fadd_rn(racc1, __shfl_xor(racc1, 16));
    racc2 = __fadd_rn(racc2, __shfl_xor(racc2, 16));
    xacc0 = __fadd_rn(xacc0, __shfl_xor(xacc0, 16));
    xacc1 = __fadd_rn(xacc1, __shfl_xor(xacc1, 16));
    xacc2 = __fadd_rn(xacc2, __shfl_xor(xacc2, 16));
    if (!ray_ok) return;
    // this lane's features: tiles 4 odd .. 4 odd + 3, register v = 4 bq + r of tile t at row
    // 32 t + 8 bq + 4 h + r
    const uint32_t tb = odd ? 4u : 0u;
    if (a.nseg > 1) {
        const size_t Rr = (size_t)G.total_tiles * kTileRays;
        float *pp = a.part + (size_t)seg * kPartQ * Rr + (size_t)tile * kTileRays + r16;
        if (a.features || a.feat_split) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int bq = 0; bq < 4; ++bq) {
                    const f4 v = facc[(4 * t + bq) * 64];
                    const uint32_t jf = 32 * (tb + t) + 8 * bq + 4 * h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pp[(size_t)(jf + r) * Rr] = v[r];
                }
        }
        if (!odd && h == 0) {
            const float q[8] = {racc0, racc1, racc2, xacc0, xacc1, xacc2, T, w_last};
#pragma unroll
            for (int k = 0; k < 8; ++k) pp[(size_t)(kW + k) * Rr] = q[k];
        }
        return;
    }
    const size_t HW = (size_t)G.H * G.W;
    const size_t pix = (size_t)py * G.W + px;
    if (!odd && h == 0) {
        a.rgb[((size_t)b * 3 + 0) * HW + pix] = __fadd_rn(-1.0f, __fmul_rn(2.0f, racc0));
        a.rgb[((size_t)b * 3 + 1) * HW + pix] = __fadd_rn(-1.0f, __fmul_rn(2.0f, racc1));
        a.rgb[((size_t)b * 3 + 2) * HW + pix] = __fadd_rn(-1.0f, __fmul_rn(2.0f, racc2));
        if (a.xyz) {
            a.xyz[((size_t)b * 3 + 0) * HW + pix] = xacc0;
            a.xyz[((size_t)b * 3 + 1) * HW + pix] = xacc1;
            a.xyz[((size_t)b * 3 + 2) * HW + pix] = xacc2;
        }
        if (a.mask) a.mask[(size_t)b * HW + pix] = w_last;
    }
    if (a.features) {
        float *fbp = a.features + (size_t)b * kW * HW + pix;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int bq = 0; bq < 4; ++bq) {
                const f4 v = facc[(4 * t + bq) * 64];
                const uint32_t jf = 32 * (tb + t) + 8 * bq + 4 * h;
#pragma unroll
                for (int r = 0; r < 4; ++r) fbp[(size_t)(jf + r) * HW] = v[r];
            }
    } else if (a.feat_split) {
        // the decoder's first input directly: v * mod[b, c] split hi / lo (fp32 product and
        // RN splits as modulate_nhwc_kernel); lanes h = 0, 1 (lane ^ 32) hold channels
        // 0-3 and 4-7 of an 8-channel group: one permlane32 swap per dword gives lane
        // h = 0 the group's 8 hi halves and lane h = 1 its 8 lo halves, one 16-B store each
        const float *fm = a.feat_mod + (size_t)b * kW;
        const size_t P = (size_t)b * HW + pix;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int bq = 0; bq < 4; ++bq) {
                const uint32_t jf = 32 * (tb + t) + 8 * bq + 4 * h;
                const f4 v = facc[(4 * t + bq) * 64] * *reinterpret_cast<const f4 *>(fm + jf);
                store_split8_pair32(a.feat_split, P * kW + (jf & ~7u), v, h);
            }
    }
}

}  // namespace sdfr

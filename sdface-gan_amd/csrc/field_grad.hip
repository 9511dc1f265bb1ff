// field_grad.hip -- the fused SDF and its exact gradient at caller-supplied points
// (sdfr_query_ngp_grad, sdfr_render_ngp_geometry, sdfr_query_siren_grad, sdfr_query_fc_grad;
// entry points in render_api.hip):
//
//   ngp_encode_grad_kernel   points [B,M,3] -> gd: per point the 32 hash-grid features and
//                            their 3 x 32 derivatives with respect to the grid coordinate u
//   field_g_kernel           forward-mode derivative of the SDF trunk (composed layer 0,
//                            pts_linears.1-2, sigma_linear) on split-fp16 MFMA: the value and
//                            its three tangents are four MFMA columns of one GEMM stream
//
// field_g_kernel is a template over the trunk (NgpGradNet here; SirenGradNet, the SIREN's
// eight FiLM layers with no gather, and FcGradNet, the FC network's eight ReLU layers on
// positional encodings, at the end of this file).  What follows describes the ngp
// instantiation; the SIREN and FC sections say what differs.
//
// Gather layout (gd): [B Mp][4 kinds][32] fp32, Mp = M rounded up to 8 (one wave pass);
// kind 0 holds the features (feature 2 level + c), kind 1 + k their derivatives d/du_k.
// 512 B per padded point; padding points and points outside [0,1]^3 hold zeros.  One
// column of the field kernel (point, kind) reads its 32 inputs as 128 contiguous bytes:
// lane half h of k-step st takes floats 16 st + 8 h .. + 7 (two 16-B loads), so the eight
// lanes of a point read its 512 B once.  The kernels index gd in fp32 elements with 32-bit
// arithmetic (128 per padded point), hence the call limit B Mp < 2^25.
//
// The value uses the rounded operations of level_interp (bit-identical to
// ngp_encode_kernel's features), the derivatives those of grid_fwd_kernel's dy_dx
// (gridencoder.cu:201-244) on the same 8 corner rows (level_value / level_dy_dx,
// sdfr_common.h): both are bit-identical to sdfr_grid_encode_forward(..., calc_dy_dx) at
// the same u, and u is formed with query_geom_kernel's three rounded ops.
//
// Field kernel: the k-step loop, the LDS-DMA weight ring and the in-register hand-off of
// activated accumulators as the next layer's B fragments are field_r_kernel's (rstep,
// field_r.h), run on the first 2 + 32 slices of the same packed weights with the same
// FiLM vectors.  A wave's 32 MFMA columns are 8 points x {value, d/du_0, d/du_1, d/du_2},
// a point's four columns in adjacent lanes (column c = 4 point + kind).  Per accumulator
// register, with z the GEMM output of the lane's own column and u = fma(gamma'', z_value,
// beta'') (revolutions) fetched from the quad's value lane by a quad-broadcast DPP move:
//     value lane     sin_rev(u)                       (field_r_kernel's arithmetic, bit for bit)
//     tangent lane   cos_rev(u) (2 pi gamma'') z      (no bias: it is folded into beta'')
// Tangents are unbounded, and the hi/lo fp16 split is fp32-accurate only inside fp16's
// range, so every tangent column is rescaled by a power of two before each split: after a
// layer's GEMM the column maximum m of |2 pi gamma'' z| over its 256 rows (an upper bound
// of the activated tangent, |cos| <= 1) gives 2^-ex(m), which brings the column into
// [-1, 1]; the cumulative exponent is carried per lane and undone exactly on the final
// sum.  The layer-0 inputs (features / derivative columns) are scaled the same way
// (field_r_kernel's es).  An all-zero column (a point outside the box) keeps exponent 0.
// The last layer's tangents feed fp32 fmas only and are not rescaled.
//
// This unit takes field_pack.h and field_r.h for their templates and helpers and
// instantiates nothing of the render's; it is built with the field kernels' flags.
#include "field_pack.h"
#include "field_r.h"

namespace sdfr {

constexpr uint32_t kGPts = kGradPts;             // points per wave pass (32 columns / 4 kinds)
constexpr uint32_t kGGroup = kGPts * kRWaves;    // points per workgroup pass
constexpr uint32_t kGPointF = 4 * kFeatIn;       // fp32 elements of gd per padded point
static_assert(kGPts == 8 && kGPointF * sizeof(float) == kGradPointBytes, "gather layout");

// ----------------------------------------------------------------------------
// gather with input derivatives
// ----------------------------------------------------------------------------
struct GGatherArgs {
    const float *points;           // [B,M,3] network coordinates
    const float *emb;
    const int32_t *offsets;
    float *gd;                     // [B Mp][4][32]
    LevelTable lt;
    uint32_t M, Mp, P;             // P = B Mp padded points
    float bound;
    int pair_ok;                   // table 16-B aligned (paired corner loads)
};

// One thread per (padded point, level), level fastest: the 16 lanes of a point store 128
// contiguous bytes per kind.
__global__ void __launch_bounds__(256) ngp_encode_grad_kernel(const GGatherArgs a) {
    __shared__ LevelParam lp[16];
    if (threadIdx.x < 16) {
        LevelParam q = a.lt.p[threadIdx.x];
        finish_level(q, a.offsets, threadIdx.x, 3, 0, 0);
        lp[threadIdx.x] = q;
    }
    __syncthreads();
    const uint32_t level = threadIdx.x & 15u;
    const uint32_t pid = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (pid >= a.P) return;
    const uint32_t b = pid / a.Mp, m = pid % a.Mp;
    float2 *out = reinterpret_cast<float2 *>(a.gd + pid * kGPointF) + level;
    bool in = m < a.M;
    float u[3] = {0.5f, 0.5f, 0.5f};
    if (in) {
        const float *p = a.points + ((size_t)b * a.M + m) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u[k] = __fdiv_rn(__fadd_rn(p[k], a.bound), __fmul_rn(2.0f, a.bound));   // grid.py:149
            if (u[k] < 0 || u[k] > 1) in = false;
        }
    }
    if (!in) {
#pragma unroll
        for (int kind = 0; kind < 4; ++kind) out[kind * 16] = make_float2(0.0f, 0.0f);
        return;
    }
    const LevelParam q = lp[level];
    const float *grid = a.emb + (size_t)q.offset * 2;
    LevelCoord<3, 2> lc;
    level_coord<3, 2>(u, q, 0, 0, lc);
    float v[8][2];
    if (a.pair_ok && !((q.offset | q.hsize) & 1u))
        level_corners<3, 2, true>(grid, q, 0, lc, v);
    else
        level_corners<3, 2, false>(grid, q, 0, lc, v);
    // value and derivatives from the same corner rows
    float res[2];
    level_value<3, 2>(lc, v, res);
    out[0] = make_float2(res[0], res[1]);
#pragma unroll
    for (uint32_t gd = 0; gd < 3; ++gd) {
        float rg[2];
        level_dy_dx<3, 2>(lc, q.scale, v, gd, rg);
        out[(1 + gd) * 16] = make_float2(rg[0], rg[1]);
    }
}

// ----------------------------------------------------------------------------
// gradient field kernel
// ----------------------------------------------------------------------------
// The SDF trunk of NgpNet: layer 0 (2 k-steps) and two dense layers (16 each) = the first
// 34 slices of NgpNet's packing; no views layer.
struct NgpGradNet {
    static constexpr int kL0 = 2;
    static constexpr int kHidden = 2;
    static constexpr int kViewSteps = 0;
    static constexpr bool kFieldR = true;
    static constexpr int kFilmN = 3;             // pts_linears.0-2
    static constexpr uint32_t kSlices = 2 + 16 * 2;
    static constexpr bool kGather = true;        // layer-0 columns from the gather's gd
    static constexpr bool kPosEnc = false;
    static constexpr uint32_t kFilmStride = kFilm;   // FiLM sets per face in `film`
};

static_assert(RNet<NgpGradNet>::kSteps == 34 && NgpGradNet::kSlices == 34, "ngp trunk k-steps");
static_assert(kGradPts * 4 == 32 && kGGroup == 32, "8 points x 4 kinds per wave, 32 per pass");

struct GFieldArgs {
    const float *gd;               // ngp: [B Mp][4][32]; siren, fc: the points [B,M,3]
    const f4 *packed;              // NgpNet's packed weights (first 34 slices read) /
                                   // SirenGradNet's (113 slices) / FcNet's (first 116 read)
    const float *film;             // [B][kFilmStride][2][256] (xprep_kernel)
    const float *sigma_w, *sigma_b;
    float *sdf;                    // [B,M] or null
    float *grad;                   // [B,M,3]
    uint32_t M, Mp, wg_per_face;
    float bound;                   // ngp only
};

__device__ __forceinline__ float quad_bcast0(float v) {   // lane n <- lane n & ~3
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x00, 0xF, 0xF, false));
}

// power-of-two exponent of a column maximum: m = f 2^ex, f in [0.5, 1); 0 for an all-zero
// or non-finite column
__device__ __forceinline__ int col_exp(float m) {
    if (!(m > 0.0f && m < 3.0e38f)) return 0;
    const int ex = __builtin_amdgcn_frexp_expf(m);
    return ex < -120 ? -120 : ex;
}

// One activated register.  MODE 0: layer 0 (the value's feature scale 2^es undone as in
// r_act), 1: a dense layer, 2: the last layer (+ the sigma head's partial dot product).
// ex: the tangent column's rescale exponent for this layer's output.
template <int MODE>
__device__ __forceinline__ float g_act1(float zz, float g, float b, float w, bool tangent, int es,
                                        int ex, float &sdfp) {
    constexpr float k2pi = 6.28318530717958647692f;
    const float uo = MODE == 0 ? __fmaf_rn(g, __builtin_ldexpf(zz, -es), b) : __fmaf_rn(g, zz, b);
    const float u = quad_bcast0(uo);
    const float sv = sin_rev(u);
    const float cv = __builtin_amdgcn_cosf(u);
    const float tv = __builtin_ldexpf(__fmul_rn(__fmul_rn(cv, __fmul_rn(k2pi, g)), zz), -ex);
    const float v = tangent ? tv : sv;
    if constexpr (MODE == 2) sdfp = __fmaf_rn(v, w, sdfp);
    return v;
}

// FcGradNet's activated register: every layer is ReLU(fma(1/su, z, b)) (r_act<.., SIN =
// false>'s arithmetic in the value lane, bit for bit).  The tangent lane takes the mask from
// the quad's value lane: u > 0 ? (1/su) z : 0 -- at u == 0 the derivative is 0, as
// torch.relu's backward has it.  MODE 2: the last layer (+ the sigma head's partial dot
// product); ex as in g_act1.
template <int MODE>
__device__ __forceinline__ float g_relu1(float zz, float g, float b, float w, bool tangent, int ex,
                                         float &sdfp) {
    const float uo = __fmaf_rn(g, zz, b);
    const float u = quad_bcast0(uo);
    const float sv = fmaxf(u, 0.0f);
    const float tv = u > 0.0f ? __builtin_ldexpf(__fmul_rn(g, zz), -ex) : 0.0f;
    const float v = tangent ? tv : sv;
    if constexpr (MODE == 2) sdfp = __fmaf_rn(v, w, sdfp);
    return v;
}

// Element e of FcGradNet's layer-0 column `kind` at ph = p / 2.  kind 0, the value column:
// posenc_val(ph, e), by the same operations (the phase offset 0 of a sine entry adds
// nothing).  kind 1 + k, the tangent column d / d p_k: with arg = RN(c_i ph_k) and
// c_i = RN32(2^i pi) as in posenc_val, + cos(arg) c_i / 2 for a sine entry and
// - sin(arg) c_i / 2 for a cosine entry of coordinate k (c_i / 2 is exact), 0 for the
// entries of the other coordinates; cos x = sin(x + pi / 2) and - sin x = sin(x + pi) go
// through posenc_val's fp64 reduction to revolutions.
__device__ __forceinline__ float posenc_col(const float (&ph)[3], uint32_t e, uint32_t kind) {
    const uint32_t i = e / 6u, r = e - 6u * i;
    const uint32_t c = r < 3u ? r : r - 3u;
    const float pc = c == 0u ? ph[0] : (c == 1u ? ph[1] : ph[2]);
    const float arg = __fmul_rn(__builtin_ldexpf(3.14159265358979323846f, (int)i), pc);
    double u = (double)arg * 0.15915494309189533577;     // 1 / (2 pi)
    u += kind == 0u ? (r >= 3u ? 0.25 : 0.0) : (r < 3u ? 0.25 : 0.5);
    u -= floor(u);
    const float s = sin_rev((float)u);
    if (kind == 0u) return s;
    return c + 1u == kind ? __fmul_rn(s, __builtin_ldexpf(3.14159265358979323846f, (int)i - 1))
                          : 0.0f;
}

template <class Net>
__global__ void __launch_bounds__(kRThreads, 1) field_g_kernel(const GFieldArgs a) {
    constexpr int NF = Net::kFilmN;
    constexpr int KL0 = Net::kL0;
    constexpr int KH = Net::kHidden;                        // the last FiLM layer (sigma head)
    constexpr int NS = RNet<Net>::kSteps;
    static_assert(NS == KL0 + 16 * KH && NS == (int)Net::kSlices, "the SDF trunk's k-steps");
    __shared__ f4 ring_lds[4 * kRSliceF4];                  // 64 KB weight ring
    __shared__ float film_lds[NF * 2 * kW];                 // the workgroup's face
    __shared__ float cst[kW];                               // sigma_w
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t c = lane & 31u, h = lane >> 5;
    const uint32_t kind = c & 3u, pt8 = c >> 2;
    const bool tangent = kind != 0u;
    const uint32_t b = blockIdx.x / a.wg_per_face, wg = blockIdx.x % a.wg_per_face;
    {
        const f4 *src = reinterpret_cast<const f4 *>(a.film + (size_t)b * Net::kFilmStride * 2 * kW);
        f4 *dst = reinterpret_cast<f4 *>(film_lds);
        for (uint32_t i = tid; i < NF * 2 * kW / 4; i += kRThreads) dst[i] = src[i];
    }
    RRing R;
    R.lds = ring_lds;
    R.tid = tid;
    R.wave = wave;
    R.ubase = 0;
    R.drsrc = make_rsrc(a.packed, Net::kSlices * kXSliceF4 * sizeof(f4));
    for (uint32_t i = tid; i < kW; i += kRThreads) cst[i] = a.sigma_w[i];
    // prologue: units 0, 1 (slices 0-3) -> slots 0-3 (unit U's barrier issues unit U + 2)
    r_dma<0>(R, 0);
    r_dma<1>(R, 1);
    r_dma<2>(R, 2);
    r_dma<3>(R, 3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const float *sig_w = cst;
    auto fg = [&](int f) { return (const float *)film_lds + f * 2 * kW; };
    auto fb = [&](int f) { return (const float *)film_lds + f * 2 * kW + kW; };
    const float sig_b = a.sigma_b[0];
    const uint32_t npass = a.Mp / kGGroup + (a.Mp % kGGroup ? 1u : 0u);

    f4 ld[4];                                               // [layer-0 k-step][16-B half]
    // this lane's point of pass p: clamped into the face for the loads
    auto point_of = [&](uint32_t p) { return (p * kRWaves + wave) * kGPts + pt8; };
    auto load_inputs = [&](uint32_t p) {
        uint32_t m = point_of(p);
        if (m >= a.M) m = a.M - 1;
        if constexpr (Net::kGather) {
            const float *src = a.gd + ((b * a.Mp + m) * 4u + kind) * kFeatIn + 8u * h;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                ld[2 * st] = *reinterpret_cast<const f4 *>(src + 16 * st);
                ld[2 * st + 1] = *reinterpret_cast<const f4 *>(src + 16 * st + 4);
            }
        } else {
            // the point itself (value column) or the unit vector e_(kind - 1) (tangent
            // columns) in K rows 0-2 of lane half 0; every other row of the k-step is zero
            const float *src = a.gd + ((size_t)b * a.M + m) * 3;
            const float px = src[0], py = src[1], pz = src[2];
            const bool h0 = h == 0u;
            if constexpr (Net::kPosEnc)
                ld[0] = f4{px, py, pz, 0.0f};               // (the columns are built per pass)
            else
                ld[0] = f4{h0 ? (kind == 0u ? px : (kind == 1u ? 1.0f : 0.0f)) : 0.0f,
                           h0 ? (kind == 0u ? py : (kind == 2u ? 1.0f : 0.0f)) : 0.0f,
                           h0 ? (kind == 0u ? pz : (kind == 3u ? 1.0f : 0.0f)) : 0.0f, 0.0f};
        }
    };
    load_inputs(wg);

    uint32_t it = 0;
    for (uint32_t p = wg; p < npass; p += a.wg_per_face, ++it) {
        R.ubase = __builtin_amdgcn_readfirstlane((it * (uint32_t)((NS + 1) / 2)) & 1u);
        r_na(R, r_slot<Net>(R, 0));
        f16v X[8], Y[8];
        f4 bf[2], bn[2], E[KL0][2];
        int es = 0;                                         // the column's layer-0 input scale
        if constexpr (Net::kGather) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[4 * k + r] = ld[k][r];
            // the column's 32 inputs over both lane halves -> 2^es into [0.5, 1)
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
            float u0[8], u1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                u0[j] = v[j];
                u1[j] = v[8 + j];
            }
            split8(u0, E[0][0], E[0][1]);
            split8(u1, E[1][0], E[1][1]);
        } else if constexpr (Net::kPosEnc) {
            // the 60 encodings of pin = RN(p / 2) (value column: unscaled, exactly the
            // render's B fragments) or their derivatives d / d p_(kind - 1) (tangent
            // columns, up to 2^9 pi / 2: scaled by 2^es into [0.5, 1) before the split);
            // this lane half's 8 of each k-step's 16, zero past 60
            const float pin[3] = {__fmul_rn(ld[0][0], 0.5f), __fmul_rn(ld[0][1], 0.5f),
                                  __fmul_rn(ld[0][2], 0.5f)};
            float v[KL0][8];
            float m = 0.0f;
#pragma unroll
            for (int st = 0; st < KL0; ++st)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t e = 16 * st + 8 * h + j;
                    v[st][j] = e < Net::kPosIn ? posenc_col(pin, e, kind) : 0.0f;
                    m = fmaxf(m, fabsf(v[st][j]));
                }
            m = fmaxf(m, __shfl_xor(m, 32));
            if (tangent && m > 0.0f && m < 3.0e38f) {
                const int ex = __builtin_amdgcn_frexp_expf(m);
                es = ex < -100 ? 100 : -ex;
            }
#pragma unroll
            for (int st = 0; st < KL0; ++st) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[st][j] = __builtin_ldexpf(v[st][j], es);
                split8(v[st], E[st][0], E[st][1]);
            }
        } else {
            // the column's 3 inputs (lane half 0; half 1 holds zeros) -> 2^es into [0.5, 1):
            // the hi / lo split is then fp32-accurate at any coordinate magnitude
            float v[8] = {ld[0][0], ld[0][1], ld[0][2], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2]));
            m = fmaxf(m, __shfl_xor(m, 32));
            if (m > 0.0f && m < 3.0e38f) {
                const int ex = __builtin_amdgcn_frexp_expf(m);
                es = ex < -100 ? 100 : -ex;
#pragma unroll
                for (int j = 0; j < 3; ++j) v[j] = __builtin_ldexpf(v[j], es);
            }
            split8(v, E[0][0], E[0][1]);
        }
        int ts = es;                                        // tangent: cumulative scale exponent
        float sdfp = 0.0f;
        struct ActState {
            f4 gm0, bt0, w0, gm1, bt1, w1;
            float v[8];
        };
        ActState as;
        auto film_load = [&](auto L, int q) {
            constexpr int l = decltype(L)::value;
            const int r0 = 32 * (q >> 1) + 16 * (q & 1) + 4 * (int)h;
            as.gm0 = *reinterpret_cast<const f4 *>(fg(l) + r0);
            as.gm1 = *reinterpret_cast<const f4 *>(fg(l) + r0 + 8);
            as.bt0 = *reinterpret_cast<const f4 *>(fb(l) + r0);
            as.bt1 = *reinterpret_cast<const f4 *>(fb(l) + r0 + 8);
            if constexpr (l == KH) {
                as.w0 = *reinterpret_cast<const f4 *>(sig_w + r0);
                as.w1 = *reinterpret_cast<const f4 *>(sig_w + r0 + 8);
            }
        };
        // register j of chunk q (registers 8 (q & 1) .. + 7 of tile q >> 1) of layer l's output
        auto act_reg = [&](auto L, f16v (&o)[8], int q, int j, int ex) {
            constexpr int l = decltype(L)::value;
            const float g = j < 4 ? as.gm0[j & 3] : as.gm1[j & 3];
            const float bb = j < 4 ? as.bt0[j & 3] : as.bt1[j & 3];
            const float w = l == KH ? (j < 4 ? as.w0[j & 3] : as.w1[j & 3]) : 0.0f;
            constexpr int MODE = l == 0 ? 0 : (l == KH ? 2 : 1);
            if constexpr (Net::kPosEnc)
                as.v[j] = g_relu1<MODE>(o[q >> 1][8 * (q & 1) + j], g, bb, w, tangent, ex, sdfp);
            else
                as.v[j] = g_act1<MODE>(o[q >> 1][8 * (q & 1) + j], g, bb, w, tangent, es, ex, sdfp);
        };
        // activation of chunk q into bn spread over a k-step's groups: film vectors read
        // beside group 0, one register beside each of groups 1-5, two beside group 6, the
        // last and the split beside group 7 (the VALU slots a 32x32 MFMA leaves free)
        auto act_side = [&](auto L, f16v (&o)[8], int q, auto GI, int ex) {
            constexpr int gi = decltype(GI)::value;
            if constexpr (gi == 0) {
                film_load(L, q);
            } else if constexpr (gi <= 5) {
                act_reg(L, o, q, gi - 1, ex);
            } else if constexpr (gi == 6) {
                act_reg(L, o, q, 5, ex);
                act_reg(L, o, q, 6, ex);
            } else {
                act_reg(L, o, q, 7, ex);
                split8(as.v, bn[0], bn[1]);
            }
        };
        auto act_now = [&](auto L, f16v (&o)[8], int q, int ex) {
            film_load(L, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) act_reg(L, o, q, j, ex);
        };
        // the tangent columns' rescale exponent for layer l's output o: the maximum of
        // |2 pi gamma'' z| over the column's 256 rows (register v of tile T: row
        // 32 T + (v & 3) + 8 (v >> 2) + 4 h), 0 in value lanes
        auto col_scale = [&](auto L, f16v (&o)[8]) {
            constexpr int l = decltype(L)::value;
            float m = 0.0f;
#pragma unroll
            for (int T = 0; T < 8; ++T)
#pragma unroll
                for (int bq = 0; bq < 4; ++bq) {
                    const f4 gm = *reinterpret_cast<const f4 *>(fg(l) + 32 * T + 8 * bq + 4 * (int)h);
#pragma unroll
                    for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(__fmul_rn(gm[r], o[T][4 * bq + r])));
                }
            m = fmaxf(m, __shfl_xor(m, 32));
            // (FcGradNet: |(1/su) z|, the ReLU's slope being at most 1)
            const int ex = col_exp(Net::kPosEnc ? m : __fmul_rn(m, 6.28318530717958647692f));
            return tangent ? ex : 0;
        };
        constexpr std::integral_constant<int, 0> L0{};
        // layer 0: K = 32 (ngp, 2 k-steps), 3 (siren, 1) or 60 (fc, 4)
        sfor<0, KL0>([&](auto J) {
            constexpr int j = decltype(J)::value;
            bf[0] = E[j][0];
            bf[1] = E[j][1];
            rstep<Net, j, j == 0>(R, X, bf, [&](auto) {});
        });
        int ex = col_scale(L0, X);
        ts -= ex;
        act_now(L0, X, 0, ex);
        split8(as.v, bn[0], bn[1]);
        // dense layers 1 .. KH (in -> out alternate X / Y), each activating the previous
        // layer's chunks one k-step ahead; the next pass's inputs are loaded under the last
        // layer's last k-steps
        auto dense = [&](auto L, f16v (&in)[8], f16v (&out)[8]) {
            constexpr int l = decltype(L)::value;
            constexpr std::integral_constant<int, l - 1> LP{};
            const bool more = p + a.wg_per_face < npass;    // (read by the last layer only)
            sfor<0, 16>([&](auto J) {
                constexpr int j = decltype(J)::value;
                bf[0] = bn[0];
                bf[1] = bn[1];
                if constexpr (l == KH && j == 12) {
                    if (more) load_inputs(p + a.wg_per_face);
                }
                rstep<Net, KL0 + 16 * (l - 1) + j, j == 0>(R, out, bf, [&](auto GI) {
                    if constexpr (j < 15) act_side(LP, in, j + 1, GI, ex);
                });
            });
            if constexpr (l < KH) {
                ex = col_scale(L, out);
                ts -= ex;
                act_now(L, out, 0, ex);
                split8(as.v, bn[0], bn[1]);
            }
        };
        sfor<1, KH + 1>([&](auto L) {
            constexpr int l = decltype(L)::value;
            if constexpr (l & 1) dense(L, X, Y);
            else dense(L, Y, X);
        });
        // last FiLM layer and sigma_linear: the value column's dot product in
        // field_r_kernel's order (chunks 0..15, registers 0..7), the tangents' likewise
        // without the bias
        f16v (&last)[8] = (KH & 1) ? Y : X;
        constexpr std::integral_constant<int, KH> LH{};
#pragma unroll
        for (int q = 0; q < 16; ++q) act_now(LH, last, q, 0);
        const float tot = __fadd_rn(sdfp, __shfl_xor(sdfp, 32));
        const uint32_t m = point_of(p);
        if (h == 0 && m < a.M) {
            const size_t o = (size_t)b * a.M + m;
            if (!tangent) {
                if (a.sdf) a.sdf[o] = __fadd_rn(tot, sig_b);
            } else {
                // ngp: d sdf / d u_k, then / (2 bound): the derivative of
                // u = (p + bound) / (2 bound); siren: the columns are d / d point already
                const float gk = __builtin_ldexpf(tot, -ts);
                a.grad[o * 3 + (kind - 1u)] =
                    Net::kGather ? __fdiv_rn(gk, __fmul_rn(2.0f, a.bound)) : gk;
            }
        }
    }
    // the ring runs ahead across passes: no LDS-DMA may land after the workgroup ends
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ----------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------
int launch_grad_gather(const sdfr_ngp_weights *w, const float *points, float *gd, uint32_t B,
                       uint32_t M, uint32_t Mp, hipStream_t st) {
    GGatherArgs e;
    e.points = points;
    e.emb = w->embeddings;
    e.offsets = w->offsets;
    e.gd = gd;
    make_level_table(16, w->log2_per_level_scale, w->base_resolution, e.lt);
    e.M = M;
    e.Mp = Mp;
    e.P = B * Mp;
    e.bound = w->bound;
    e.pair_ok = (reinterpret_cast<uintptr_t>(w->embeddings) & 15u) == 0;
    hipLaunchKernelGGL(ngp_encode_grad_kernel, dim3((e.P + 15) / 16), dim3(256), 0, st, e);
    return check_launch("query_ngp_grad: gather");
}

// The forward-mode field kernel of a trunk.  xws: the packed weights' region (workspace or
// the caller's prepacked buffer); in: the ngp gather's gd or the SIREN's points.
template <class Net>
static int launch_gfield_net(const NetPtrs &P, const char *xws, const float *film,
                             const float *in, float *sdf, float *grad, uint32_t B, uint32_t M,
                             float bound, const char *what, hipStream_t st) {
    GFieldArgs f{};
    f.gd = in;
    f.packed = reinterpret_cast<const f4 *>(xws);
    f.film = film;
    f.sigma_w = P.sigma_w;
    f.sigma_b = P.sigma_b;
    f.sdf = sdf;
    f.grad = grad;
    f.M = M;
    f.Mp = (M + kGradPts - 1) / kGradPts * kGradPts;
    f.bound = bound;
    // workgroups of a face take its passes (32 points each) round robin: about four
    // workgroups per CU over the call, every workgroup at least one pass
    const uint32_t npass = (f.Mp + kGGroup - 1) / kGGroup;
    const uint32_t want = (1024u + B - 1) / B;
    f.wg_per_face = npass < want ? npass : want;
    hipLaunchKernelGGL(field_g_kernel<Net>, dim3(B * f.wg_per_face), dim3(kRThreads), 0, st, f);
    return check_launch(what);
}

// ----------------------------------------------------------------------------
// SIREN: the SDF and its gradient at caller points (sdfr_query_siren_grad)
//
//   xprep_kernel<SirenGradNet>    FiLM vectors of the faces' styles and (once per weight
//                                 version: sdfr_query_siren_grad_pack) the trunk's weights
//                                 in field_r_kernel's packing
//   field_g_kernel<SirenGradNet>  the forward-mode kernel over pts_linears.0-7 and
//                                 sigma_linear
//
// There is no gather: layer 0's value column is the point (x, y, z, 0, ...) and tangent
// column k the unit vector e_k, both scaled by a power of two into [0.5, 1) before the
// hi / lo split as the ngp columns are.  FiLM gamma is about 30, so a tangent grows by
// orders of magnitude per layer: the per-layer power-of-two rescale, which the ngp
// trunk's two layers barely need, is what keeps the seven dense layers' tangent columns
// inside fp16's range.  Instantiated beside the ngp kernel: this unit's ngp kernels come
// out of the compiler unchanged with it (profiles/siren_query_isa.txt).
// ----------------------------------------------------------------------------
// The SDF trunk of SirenNet (pts_linears.0-7, sigma_linear): layer 0 (one k-step on the
// point itself) and seven dense layers, in field_r_kernel's packing -- one slice per
// k-step of 16 K, K permuted by rperm_k.  The render's SIREN packing is field_p_kernel's
// (half-slices per k-step of 32 K), so this trunk is packed on its own
// (sdfr_query_siren_grad_pack: xprep_kernel<SirenGradNet>, r_pack).  kLayers counts a
// views layer of zero k-steps so that rslice_base / rperm_k index the dense layers as they
// do for the render policies; there are eight weight matrices and eight FiLM sets.
struct SirenGradNet {
    static constexpr bool kSiren = true;
    static constexpr bool kGrid = false;
    static constexpr bool kPosEnc = false;
    static constexpr bool kSinAct = true;
    static constexpr int kL0 = 1;
    static constexpr int kHidden = 7;
    static constexpr int kViewSteps = 0;
    static constexpr bool kFieldR = true;
    static constexpr bool kQuery = false;
    static constexpr bool kCompose = false;
    static constexpr int kLayers = 9;            // pts_linears.0-7 (+ the absent views layer)
    static constexpr int kMats = 8;              // weight matrices, row scales, FiLM sets
    static constexpr int kFilmN = 8;
    static constexpr uint32_t kSlices = 1 + 16 * 7;
    static constexpr bool kGather = false;       // layer-0 columns: the point and unit vectors
    static constexpr uint32_t kFilmStride = 8;
    __host__ __device__ static constexpr uint32_t K(int l) { return l == 0 ? 3u : kW; }
    __host__ __device__ static constexpr int film_layer(int f) { return f; }
};
static_assert(RNet<SirenGradNet>::kSteps == 113 && SirenGradNet::kSlices == 113 &&
                  rslice_base<SirenGradNet>(7) == 97,
              "siren trunk: one slice per k-step, dense layer l at 1 + 16 (l - 1)");

// ----------------------------------------------------------------------------
// SIREN host side
// ----------------------------------------------------------------------------
size_t siren_grad_pack_bytes() {
    return (size_t)SirenGradNet::kSlices * kRSliceF4 * sizeof(f4) +
           2 * (size_t)SirenGradNet::kMats * kW * sizeof(float);
}

static_assert(SirenGradNet::kFilmN == kSirenGradFilm, "the entry point sizes film with this");

// xprep_kernel on the trunk's eight matrices (P.w[0..7] = pts_linears): launch_xpack's
// (field_f16x3.hip) steps, with the su | bias_s stride of kMats = 8 rows, not kLayers.
int launch_gprep_siren(const NetPtrs &P, uint32_t B, const float *styles, char *xws, float *film,
                       bool pack, hipStream_t st) {
    using Net = SirenGradNet;
    float *su = reinterpret_cast<float *>(xws + (size_t)Net::kSlices * kRSliceF4 * sizeof(f4));
    if (pack) {
        uint32_t K[Net::kMats];
        for (int l = 0; l < Net::kMats; ++l) K[l] = Net::K(l);
        int rc = launch_xscale(P.w, P.b, K, Net::kMats, su, su + Net::kMats * kW, st);
        if (rc) return rc;
    }
    XPrepArgs p{};
    p.styles = styles;
    for (int l = 0; l < Net::kMats; ++l) {
        p.gw[l] = P.gw[l];
        p.gb[l] = P.gb[l];
        p.bw[l] = P.bw[l];
        p.bb[l] = P.bb[l];
        p.w[l] = P.w[l];
        p.lb[l] = P.b[l];
    }
    p.su = su;
    p.film = film;
    p.packed = reinterpret_cast<f4 *>(xws);
    p.B = film ? B : 0;
    const uint32_t nfilm = p.B * Net::kFilmN * 2 * kW / 4;
    const uint32_t blocks = nfilm + (pack ? (Net::kSlices * 512 + 255) / 256 : 0);
    if (blocks == 0) return SDFR_OK;
    hipLaunchKernelGGL(xprep_kernel<Net>, dim3(blocks), dim3(256), 0, st, p);
    return check_launch("query_siren_grad: xprep");
}

// ----------------------------------------------------------------------------
// FC: the SDF and its gradient at caller points (sdfr_query_fc_grad)
//
//   xprep_kernel<FcNet>         the render's FiLM slots and packing (launch_xprep)
//   field_g_kernel<FcGradNet>   the forward-mode kernel over x_in, pts_linears.0-6 and
//                               sigma_linear
//
// FcNet is a field_r_kernel policy with the views layer packed last, so its SDF trunk is
// the first 4 + 16 x 7 = 116 slices of the render's own packing, as ngp's is the first 34
// of its: no packing of its own.  Layer 0's columns are built in the kernel (posenc_col):
// the value column holds the render's 60 encodings unscaled, so with the same slices in
// the same k-step order the value lanes repeat the query's arithmetic and `sdf` is the
// query's bit for bit; tangent column k holds the encodings' derivatives d / d p_k, up to
// 2^9 pi / 2, scaled by a power of two before the split.  Every layer is ReLU: the tangent
// lane passes (1/su) z where the quad's value lane has u > 0 (g_relu1).  The per-layer
// power-of-two rescale of the tangent columns is the other trunks'; it also carries
// gradients far below fp16's range (a trunk whose late layers are nearly dead).
// ----------------------------------------------------------------------------
struct FcGradNet {
    static constexpr bool kPosEnc = true;
    static constexpr int kL0 = 4;                // 60 encodings (+ 4 zero pad)
    static constexpr int kHidden = 7;
    static constexpr int kViewSteps = 0;
    static constexpr bool kFieldR = true;
    static constexpr int kFilmN = 8;             // x_in, pts_linears.0-6
    static constexpr uint32_t kSlices = 4 + 16 * 7;
    static constexpr bool kGather = false;       // layer-0 columns from the point itself
    static constexpr uint32_t kFilmStride = kFcFilm;   // the render's sets per face
    static constexpr uint32_t kPosIn = FcNet::kPosIn;
};
static_assert(RNet<FcGradNet>::kSteps == 116 && FcGradNet::kSlices == 116 &&
                  FcGradNet::kL0 == FcNet::kL0 && FcGradNet::kHidden == FcNet::kHidden &&
                  rslice_base<FcNet>(FcNet::kLayers - 1) == 116,
              "fc trunk: the render's slices ahead of its views layer");

int launch_gfield(int net, const NetPtrs &P, const char *xws, const float *film, const float *in,
                  float *sdf, float *grad, uint32_t B, uint32_t M, float bound, hipStream_t st) {
    if (net == kNetNgp)
        return launch_gfield_net<NgpGradNet>(P, xws, film, in, sdf, grad, B, M, bound,
                                             "query_ngp_grad: field (f16x3)", st);
    if (net == kNetFc)
        return launch_gfield_net<FcGradNet>(P, xws, film, in, sdf, grad, B, M, 0.0f,
                                            "query_fc_grad: field (f16x3)", st);
    return launch_gfield_net<SirenGradNet>(P, xws, film, in, sdf, grad, B, M, 0.0f,
                                           "query_siren_grad: field (f16x3)", st);
}

}  // namespace sdfr

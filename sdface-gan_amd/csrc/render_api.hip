// render_api.hip -- the C entry points of the fused renderer (include/sdfr.h): the render of
// the three networks (ngp, SIREN, FC), the field query and the SDF gradient at caller points
// (ngp, SIREN, FC), the ngp geometry render, the surface render (ngp, SIREN), and their packing
// and workspace-size calls.
//
// Host code only.  An entry point checks its arguments, lays out its workspace and enqueues
// the stages in order on the caller's stream through the launch functions the kernel units
// export (render_launch.h); no kernel is launched from this file.  What the calls share is
// written once here: the checks of sdfr_ngp_render_args, one weight check per network, the
// workspace layouts (one function per call from its sizes to named offsets, called once),
// the choice between weights packed beforehand and packing inside the workspace, and the
// network's tensors in the field kernels' order (NetPtrs).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>

#include "render_launch.h"

namespace sdfr {
namespace {

int err(const char *who, int code, const char *what) {
    return fail(code, std::string(who) + ": " + what);
}

void record_event(void *ev, hipStream_t st) {
    if (ev) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(ev), st);
}

// stream waits on a caller's hipEvent_t (NULL: nothing)
void wait_event(void *ev, hipStream_t st) {
    if (ev) (void)hipStreamWaitEvent(st, reinterpret_cast<hipEvent_t>(ev), 0);
}

// ----------------------------------------------------------------------------
// workspace layouts: consecutive regions, each rounded up to 256 bytes
// ----------------------------------------------------------------------------
struct Regions {
    size_t off = 0;
    size_t take(size_t bytes) {            // the region's offset
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

size_t film_bytes(uint32_t B, uint32_t films) { return (size_t)B * films * 2 * kW * sizeof(float); }
uint32_t tiles_of(uint32_t H, uint32_t W) { return (H * W + kTileRays - 1) / kTileRays; }

// ngp render: enc [L][S][2] (at 0) | packed fp32 fragments | film | split-fp16 region |
// segment partials | zd [S] (z, segment length) | gu [S] (grid coordinate, inside flag)
struct NgpRenderWs {
    uint64_t S;                                // padded samples
    size_t packed, film, x, part, zd, gu, total;
};
NgpRenderWs ngp_render_ws(uint32_t B, uint32_t H, uint32_t W, uint32_t N, uint32_t L) {
    const size_t S = (size_t)B * tiles_of(H, W) * N * kTileRays;
    Regions r;
    NgpRenderWs l;
    l.S = S;
    r.take(S * L * 2 * sizeof(float));
    l.packed = r.take(fp32_packed_bytes());
    l.film = r.take(film_bytes(B, kFilm));
    l.x = r.take(f16x3_ws_bytes(kNetNgp));
    l.part = r.take(field_part_bytes(B, tiles_of(H, W), N));
    l.zd = r.take(S * 2 * sizeof(float));
    l.gu = r.take(S * 4 * sizeof(float));
    l.total = r.off;
    return l;
}

// SIREN and FC calls: film [B][films][2][256] (at 0) | weight region | segment partials
// (FC render only).  total 0: too many points (the SIREN point calls).
struct FilmWs {
    size_t x, part, total;
};
FilmWs film_ws(uint32_t B, uint32_t films, size_t x_bytes, size_t part_bytes) {
    Regions r;
    FilmWs l;
    r.take(film_bytes(B, films));
    l.x = r.take(x_bytes);
    l.part = r.take(part_bytes);
    l.total = r.off;
    return l;
}
FilmWs f16x3_render_ws(int net, uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    if (net == kNetSiren) return film_ws(B, kSirenFilm, f16x3_ws_bytes(net), 0);
    return film_ws(B, kFcFilm, f16x3_ws_bytes(net), field_part_bytes(B, tiles_of(H, W), N));
}

// ngp query: enc [16][S][2] (at 0) | film [B][4][2][256] | split-fp16 region | gu [S];
// S = B x (R rounded up to 16) x N padded samples
struct NgpQueryWs {
    uint64_t S;
    size_t film, x, gu, total;
};
NgpQueryWs ngp_query_ws(uint32_t B, uint32_t R, uint32_t N) {
    Regions r;
    NgpQueryWs l;
    l.S = (uint64_t)B * (((uint64_t)R + kTileRays - 1) / kTileRays) * N * kTileRays;
    r.take((size_t)l.S * 16 * 2 * sizeof(float));
    l.film = r.take(film_bytes(B, kFilm));
    l.x = r.take(f16x3_ws_bytes(kNetNgp));
    l.gu = r.take((size_t)l.S * 4 * sizeof(float));
    l.total = r.off;
    return l;
}

// ngp gradient: gd [B Mp][4][32] (at 0) | film [B][4][2][256] | split-fp16 region; Mp = M
// rounded up to 8.  The kernels index gd in fp32 elements, 128 per padded point, with
// 32-bit arithmetic: P = B Mp >= 2^25 is too many points for one call (P < 2^64: B < 2^32,
// Mp <= 2^32), and gives total 0 before any byte size is formed.
constexpr uint64_t kGradMaxPoints = (1ull << 32) / (kGradPointBytes / sizeof(float));
struct NgpGradWs {
    uint64_t P;
    size_t film, x, total;
};
NgpGradWs ngp_grad_ws(uint32_t B, uint32_t M) {
    const uint64_t Mp = ((uint64_t)M + kGradPts - 1) / kGradPts * kGradPts;
    NgpGradWs l{};
    l.P = (uint64_t)B * Mp;
    if (l.P >= kGradMaxPoints) return l;
    Regions r;
    r.take((size_t)l.P * kGradPointBytes);
    l.film = r.take(film_bytes(B, kFilm));
    l.x = r.take(f16x3_ws_bytes(kNetNgp));
    l.total = r.off;
    return l;
}

// geometry render: the gradient call's workspace for (B, M = H W N) | pnet [P][3] | zd [P]
// (z, dist) | sdf [P] | gnet [P][3]; P = B Mp padded points, 36 bytes more per padded point.
// M >= 2^25 alone is too many points (H W N is formed in steps that cannot wrap): total 0.
struct NgpGeomWs {
    uint32_t M;
    NgpGradWs g;
    size_t pnet, zd, sdf, gnet, total;
};
NgpGeomWs ngp_geom_ws(uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    NgpGeomWs l{};
    const uint64_t HW = (uint64_t)H * W;
    if (HW >= kGradMaxPoints || HW * N >= kGradMaxPoints) return l;
    l.M = (uint32_t)(HW * N);
    l.g = ngp_grad_ws(B, l.M);
    if (l.g.total == 0) return l;
    Regions r{l.g.total};
    l.pnet = r.take((size_t)l.g.P * 3 * sizeof(float));
    l.zd = r.take((size_t)l.g.P * 2 * sizeof(float));
    l.sdf = r.take((size_t)l.g.P * sizeof(float));
    l.gnet = r.take((size_t)l.g.P * 3 * sizeof(float));
    l.total = r.off;
    return l;
}

// SIREN point calls (query, gradient).  The kernels form 3 x (point index) in 32 bits, so a
// call takes fewer than 2^30 padded points.  The query's padded count is
// S = B x (R rounded up to 16) x N, formed in steps that cannot wrap 64 bits (0: too many);
// the gradient's is P = B x (M rounded up to 8) < 2^64.
constexpr uint64_t kSirenMaxPoints = 1ull << 30;
uint64_t siren_query_padded(uint32_t B, uint32_t R, uint32_t N) {
    const uint64_t Rp = ((uint64_t)R + kTileRays - 1) / kTileRays * kTileRays;
    if (Rp >= kSirenMaxPoints || (uint64_t)B * Rp >= kSirenMaxPoints) return 0;
    const uint64_t S = (uint64_t)B * Rp * N;
    return S >= kSirenMaxPoints ? 0 : S;
}

// gradient: film [B][8][2][256] | the trunk's packing (siren_grad_pack_bytes)
FilmWs siren_grad_ws(uint32_t B, uint32_t M) {
    const uint64_t P = (uint64_t)B * (((uint64_t)M + kGradPts - 1) / kGradPts * kGradPts);
    if (P == 0 || P >= kSirenMaxPoints) return FilmWs{};
    return film_ws(B, kSirenGradFilm, siren_grad_pack_bytes(), 0);
}

// FC point calls (query, gradient): film [B][9][2][256] | the render's weight region -- the
// FC render's workspace without segment partials.  The kernels index the points as the
// SIREN's do, so the padded counts and their limit are the SIREN calls' (total 0: too many).
FilmWs fc_query_ws(uint32_t B, uint32_t R, uint32_t N) {
    if (siren_query_padded(B, R, N) == 0) return FilmWs{};
    return film_ws(B, kFcFilm, f16x3_ws_bytes(kNetFc), 0);
}
FilmWs fc_grad_ws(uint32_t B, uint32_t M) {
    const uint64_t P = (uint64_t)B * (((uint64_t)M + kGradPts - 1) / kGradPts * kGradPts);
    if (P == 0 || P >= kSirenMaxPoints) return FilmWs{};
    return film_ws(B, kFcFilm, f16x3_ws_bytes(kNetFc), 0);
}

// surface render (net: kNetNgp or kNetSiren).  With M = H W rays per face, Mp = M rounded up
// to 32 (the refinement points, in the query's groups of 32), S = B M N, rays = B M and
// P = B Mp:
//   q     the SDF / colour evaluations' sub-workspace.  ngp: the query call's layout for the
//         largest padded point count per face of its three shapes, Pq = max((M up to 16) N,
//         (Mp / 32 up to 16) 32) -- ngp_query_ws(B, 16, Pq / 16); SIREN: the query call's
//   g     the gradient call's sub-workspace for (B, M)
//   pnet [S][3] | zd [S] (z, dist) | sdf [S] | br [rays] (a, b, fa, fb) | sidx [rays] |
//   zs [rays] | pts [P][3] | f [P] | hitp [rays][3] | dirs [rays][3] | gsdf [rays] |
//   ggrad [rays][3] | csdf [rays] | rgbq [rays][3]
// total 0: too many points.  The coarse pass is the binding count: M N (and Pq, B Pq) must
// stay below 2^25 padded points for ngp (the query's and the gradient's 32-bit indexing) and
// below 2^30 for SIREN, the products formed in steps that cannot wrap 64 bits.
struct SurfWs {
    uint32_t M, Mp;
    NgpQueryWs nq;
    NgpGradWs ng;
    FilmWs sq, sg;
    size_t q, g, pnet, zd, sdf, br, sidx, zs, pts, f, hitp, dirs, gsdf, ggrad, csdf, rgbq, total;
};
SurfWs surf_ws(int net, uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    SurfWs l{};
    const uint64_t lim = net == kNetNgp ? kGradMaxPoints : kSirenMaxPoints;
    const uint64_t M = (uint64_t)H * W;
    if (B == 0 || M == 0 || N == 0 || M >= lim || M * N >= lim) return l;
    const uint64_t Mp = (M + 31) / 32 * 32;
    const uint64_t coarse = (M + kTileRays - 1) / kTileRays * kTileRays * N;       // < 2^63
    const uint64_t refine = (Mp / 32 + kTileRays - 1) / kTileRays * kTileRays * 32;
    const uint64_t Pq = coarse > refine ? coarse : refine;
    if (Pq >= lim || (uint64_t)B * Pq >= lim) return l;
    l.M = (uint32_t)M;
    l.Mp = (uint32_t)Mp;
    Regions r;
    if (net == kNetNgp) {
        l.nq = ngp_query_ws(B, kTileRays, (uint32_t)(Pq / kTileRays));
        l.ng = ngp_grad_ws(B, l.M);
        l.q = r.take(l.nq.total);
        l.g = r.take(l.ng.total);
    } else {
        l.sq = f16x3_render_ws(kNetSiren, B, 0, 0, 0);
        l.sg = siren_grad_ws(B, l.M);
        l.q = r.take(l.sq.total);
        l.g = r.take(l.sg.total);
    }
    const size_t S = (size_t)B * M * N, rays = (size_t)B * M, P = (size_t)B * Mp, f = sizeof(float);
    l.pnet = r.take(S * 3 * f);
    l.zd = r.take(S * 2 * f);
    l.sdf = r.take(S * f);
    l.br = r.take(rays * 4 * f);
    l.sidx = r.take(rays * f);
    l.zs = r.take(rays * f);
    l.pts = r.take(P * 3 * f);
    l.f = r.take(P * f);
    l.hitp = r.take(rays * 3 * f);
    l.dirs = r.take(rays * 3 * f);
    l.gsdf = r.take(rays * f);
    l.ggrad = r.take(rays * 3 * f);
    l.csdf = r.take(rays * f);
    l.rgbq = r.take(rays * 3 * f);
    l.total = r.off;
    return l;
}

// The split-fp16 weight region of a call: the caller's buffer, packed beforehand
// (sdfr_render_*_pack, sdfr_query_siren_grad_pack), or else the workspace's own region,
// which the call then packs itself (launch_xprep / launch_gprep_siren with pack).
char *weight_region(const void *prepacked, char *ws_region) {
    return prepacked ? const_cast<char *>(reinterpret_cast<const char *>(prepacked)) : ws_region;
}

// ----------------------------------------------------------------------------
// argument checks (`who` prefixes the message)
// ----------------------------------------------------------------------------
bool any_null(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!p) return true;
    return false;
}

// sdfr_ngp_render_args, for the three render calls (allow_fp32: the ngp render's fp32 field)
template <class Weights>
int check_render_args(const Weights *w, const sdfr_ngp_render_args *a, const char *who,
                      bool allow_fp32) {
    if (!w || !a) return err(who, SDFR_EINVAL, "null args");
    if (a->B == 0 || a->H == 0 || a->W == 0 || a->N == 0)
        return err(who, SDFR_EINVAL, "empty batch / image / sample count");
    if (!allow_fp32 && a->field_precision != SDFR_FIELD_F16X3)
        return err(who, SDFR_EUNSUPPORTED, "only field_precision 0 (f16x3)");
    if (a->field_precision != SDFR_FIELD_F16X3 && a->field_precision != SDFR_FIELD_FP32)
        return err(who, SDFR_EINVAL, "field_precision must be 0 (f16x3) or 1 (fp32)");
    if (a->max_field_segments > kFieldSplitMax || a->max_field_segments == 3)
        return err(who, SDFR_EINVAL, "max_field_segments must be 0, 1, 2 or 4");
    if (any_null({a->cam, a->focal, a->near_, a->far_, a->styles, a->pix_x, a->pix_y, a->t_vals,
                  a->rgb, a->workspace}))
        return err(who, SDFR_EINVAL, "required pointer is null");
    if (a->with_sdf && !w->sigmoid_beta)
        return err(who, SDFR_EINVAL, "sigmoid_beta is required when with_sdf");
    return SDFR_OK;
}

// FiLM layer l of the ngp / SIREN weights: the linear layer and its gamma / beta maps
template <class Weights>
bool film_layer_null(const Weights *w, int l) {
    return any_null({w->pts_w[l], w->pts_b[l], w->pts_gw[l], w->pts_gb[l], w->pts_bw[l],
                     w->pts_bb[l]});
}

// The network's shape and weight pointers, for every entry point that takes the network's
// weight struct (need_rgb / colour: the colour layers are read too).
int check_ngp_weights(const sdfr_ngp_weights *w, const char *who, bool need_rgb) {
    if (w->num_levels != 16)
        return err(who, SDFR_EUNSUPPORTED, "fused path needs 16 levels x 2 features");
    if (any_null({w->embeddings, w->offsets, w->input_w, w->input_b, w->views_w, w->views_b,
                  w->views_gw, w->views_gb, w->views_bw, w->views_bb, w->sigma_w, w->sigma_b}) ||
        (need_rgb && any_null({w->rgb_w, w->rgb_b})))
        return err(who, SDFR_EINVAL, "weight pointer is null");
    for (int l = 0; l < 3; ++l)
        if (film_layer_null(w, l)) return err(who, SDFR_EINVAL, "FiLM weight pointer is null");
    return SDFR_OK;
}

int check_siren_weights(const sdfr_siren_weights *w, const char *who, bool colour) {
    if (w->depth != 8 || w->width != 256)
        return err(who, SDFR_EUNSUPPORTED, "fused path needs depth 8, width 256");
    for (int l = 0; l < 8; ++l)
        if (film_layer_null(w, l)) return err(who, SDFR_EINVAL, "FiLM weight pointer is null");
    if (any_null({w->sigma_w, w->sigma_b}) ||
        (colour && any_null({w->views_w, w->views_b, w->views_gw, w->views_gb, w->views_bw,
                             w->views_bb, w->rgb_w, w->rgb_b})))
        return err(who, SDFR_EINVAL, "weight pointer is null");
    return SDFR_OK;
}

int check_fc_weights(const sdfr_fc_weights *w, const char *who) {
    if (w->depth != 8 || w->width != 256)
        return err(who, SDFR_EUNSUPPORTED, "fused path needs depth 8, width 256");
    bool null = any_null({w->x_in_w, w->x_in_b, w->style_w, w->style_b, w->views_w, w->views_b,
                          w->sigma_w, w->sigma_b, w->rgb_w, w->rgb_b});
    for (int l = 0; l < 7; ++l) null |= any_null({w->pts_w[l], w->pts_b[l]});
    return null ? err(who, SDFR_EINVAL, "weight pointer is null") : SDFR_OK;
}

// the sizes and pointers of a query / gradient call (one argument struct for the three
// networks)
int check_query_args(const void *w, const sdfr_query_args *a, const char *who) {
    if (!w || !a) return err(who, SDFR_EINVAL, "null args");
    if (a->B == 0 || a->R == 0 || a->N == 0)
        return err(who, SDFR_EINVAL, "empty batch / group / point count");
    if (any_null({a->points, a->dirs, a->styles, a->sdf, a->workspace}))
        return err(who, SDFR_EINVAL, "required pointer is null");
    return SDFR_OK;
}

int check_grad_args(const void *w, const sdfr_grad_args *a, const char *who) {
    if (!w || !a) return err(who, SDFR_EINVAL, "null args");
    if (a->B == 0 || a->M == 0) return err(who, SDFR_EINVAL, "empty batch / point count");
    if (any_null({a->points, a->styles, a->grad, a->workspace}))
        return err(who, SDFR_EINVAL, "required pointer is null");
    return SDFR_OK;
}

// ----------------------------------------------------------------------------
// the networks' tensors in the field kernels' order
// ----------------------------------------------------------------------------
template <class Weights>
void head_ptrs(const Weights *w, NetPtrs &P) {
    P.sigma_w = w->sigma_w;
    P.sigma_b = w->sigma_b;
    P.rgb_w = w->rgb_w;
    P.rgb_b = w->rgb_b;
    P.sigmoid_beta = w->sigmoid_beta;
}

// FiLM set l of the policy: the maps of pts_linears.l (ngp, SIREN)
template <class Weights>
void film_ptrs(const Weights *w, int l, NetPtrs &P) {
    P.gw[l] = w->pts_gw[l];
    P.gb[l] = w->pts_gb[l];
    P.bw[l] = w->pts_bw[l];
    P.bb[l] = w->pts_bb[l];
}

// layer `l` and FiLM set `l` of the policy: the views layer of the ngp / SIREN weights
template <class Weights>
void views_ptrs(const Weights *w, int l, NetPtrs &P) {
    P.w[l] = w->views_w;
    P.b[l] = w->views_b;
    P.gw[l] = w->views_gw;
    P.gb[l] = w->views_gb;
    P.bw[l] = w->views_bw;
    P.bb[l] = w->views_bb;
}

NetPtrs ngp_ptrs(const sdfr_ngp_weights *w) {
    NetPtrs P{};
    P.in_w = w->input_w;                       // composed into layer 0 (launch_xprep)
    P.in_b = w->input_b;
    P.p0_w = w->pts_w[0];
    P.p0_b = w->pts_b[0];
    for (int l = 1; l < 3; ++l) {
        P.w[l] = w->pts_w[l];
        P.b[l] = w->pts_b[l];
    }
    for (int l = 0; l < 3; ++l) film_ptrs(w, l, P);
    views_ptrs(w, 3, P);
    head_ptrs(w, P);
    return P;
}

NetPtrs siren_ptrs(const sdfr_siren_weights *w) {
    NetPtrs P{};
    for (int l = 0; l < 8; ++l) {
        P.w[l] = w->pts_w[l];
        P.b[l] = w->pts_b[l];
        film_ptrs(w, l, P);
    }
    views_ptrs(w, 8, P);
    head_ptrs(w, P);
    return P;
}

NetPtrs fc_ptrs(const sdfr_fc_weights *w) {
    NetPtrs P{};
    P.w[0] = w->x_in_w;
    P.b[0] = w->x_in_b;
    P.gw[0] = w->style_w;                      // style_in: layer 0's per-face bias
    P.gb[0] = w->style_b;
    for (int l = 0; l < 7; ++l) {
        P.w[1 + l] = w->pts_w[l];
        P.b[1 + l] = w->pts_b[l];
    }
    P.w[8] = w->views_w;
    P.b[8] = w->views_b;
    head_ptrs(w, P);
    return P;
}

// ----------------------------------------------------------------------------
// ray / sample geometry arguments
// ----------------------------------------------------------------------------
// the camera / sampling fields of a render or geometry call (sdfr_ngp_render_args,
// sdfr_ngp_geometry_args: the shared fields have the same names)
template <class Args>
GeomArgs camera_geom(const Args *a, int static_viewdirs, float bound) {
    GeomArgs g;
    g.B = a->B;
    g.H = a->H;
    g.W = a->W;
    g.N = a->N;
    g.tiles_per_face = tiles_of(a->H, a->W);
    g.total_tiles = a->B * g.tiles_per_face;
    g.S_total = g.total_tiles * a->N * kTileRays;
    g.half_res = (float)a->W * 0.5f;   // get_rays uses out_im_res * .5 for both axes
    g.cam = a->cam;
    g.focal = a->focal;
    g.near_ = a->near_;
    g.far_ = a->far_;
    g.pix_x = a->pix_x;
    g.pix_y = a->pix_y;
    g.sc.t_vals = a->t_vals;
    g.sc.t_rand = a->t_rand;
    g.sc.t_rand_per_sample = a->t_rand_per_sample;
    g.sc.offset_sampling = a->offset_sampling;
    g.sc.N = a->N;
    g.static_viewdirs = static_viewdirs;
    g.z_normalize = a->z_normalize;
    g.bound = bound;
    return g;
}

// a point query in the field kernels' terms: H = 1, W = R direction groups of N points,
// S padded samples in tile order, the groups' directions dirs [B,R,3] in place of a camera
GeomArgs query_geom(uint32_t B, uint32_t R, uint32_t N, uint64_t S, const float *dirs,
                    float bound) {
    GeomArgs g{};
    g.B = B;
    g.H = 1;
    g.W = R;
    g.N = N;
    g.tiles_per_face = tiles_of(1, R);
    g.total_tiles = B * g.tiles_per_face;
    g.S_total = (uint32_t)S;
    g.cam = dirs;
    g.bound = bound;
    return g;
}

// ----------------------------------------------------------------------------
// the SIREN and FC render: FiLM prep, then the field kernel (no encode stage)
// ----------------------------------------------------------------------------
int render_f16x3(int net, const char *who, const NetPtrs &P, const sdfr_ngp_render_args *a,
                 hipStream_t st) {
    const FilmWs l = f16x3_render_ws(net, a->B, a->H, a->W, a->N);
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *film = reinterpret_cast<float *>(ws);
    char *xws = weight_region(a->prepacked, ws + l.x);
    // the sample-segment partials: field_r_kernel (FC) only
    float *part = net == kNetFc ? reinterpret_cast<float *>(ws + l.part) : nullptr;
    const GeomArgs g = camera_geom(a, a->static_viewdirs, 1.0f);
    int rc;
    record_event(a->stage_events[0], st);
    wait_event(a->styles_event, st);
    if ((rc = launch_xprep(net, P, a->B, a->styles, xws, film, !a->prepacked, st))) return rc;
    record_event(a->stage_events[1], st);
    record_event(a->stage_events[2], st);
    record_event(a->field_event, st);
    if ((rc = launch_xfield(net, P, a, g, nullptr, xws, film, st, part, nullptr))) return rc;
    record_event(a->stage_events[3], st);
    return SDFR_OK;
}

// the ngp gradient's stages on points [B,M,3]: gather, FiLM prep, forward-mode field kernel
int ngp_gradient(const sdfr_ngp_weights *w, uint32_t B, uint32_t M, const float *points,
                 const float *styles, const void *prepacked, char *ws, const NgpGradWs &l,
                 float *sdf, float *grad, hipStream_t st) {
    float *gd = reinterpret_cast<float *>(ws);
    float *film = reinterpret_cast<float *>(ws + l.film);
    char *xws = weight_region(prepacked, ws + l.x);
    const NetPtrs P = ngp_ptrs(w);
    int rc;
    if ((rc = launch_grad_gather(w, points, gd, B, M, (uint32_t)(l.P / B), st))) return rc;
    if ((rc = launch_xprep(kNetNgp, P, B, styles, xws, film, !prepacked, st))) return rc;
    return launch_gfield(kNetNgp, P, xws, film, gd, sdf, grad, B, M, w->bound, st);
}

// the ngp render's checks; the workspace layout of an accepted call in `l`
int check_ngp_render(const sdfr_ngp_weights *w, const sdfr_ngp_render_args *a, NgpRenderWs &l) {
    const char *who = "render_ngp";
    int rc = check_render_args(w, a, who, true);
    if (rc || (rc = check_ngp_weights(w, who, true))) return rc;
    if (a->features_split) {
        if (a->field_precision != SDFR_FIELD_F16X3)
            return err(who, SDFR_EUNSUPPORTED, "features_split needs the f16x3 field");
        if (a->features || !a->features_mod)
            return err(who, SDFR_EINVAL, "features_split takes features_mod and no features");
    }
    l = ngp_render_ws(a->B, a->H, a->W, a->N, 16);
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");
    if (l.S * 16 >= (1ull << 32))
        return err(who, SDFR_EINVAL, "too many samples per call (split the batch)");
    return SDFR_OK;
}

// ----------------------------------------------------------------------------
// the surface render's host path, shared by the two networks (SurfNet: what differs)
// ----------------------------------------------------------------------------
struct NgpSurf {
    using Weights = sdfr_ngp_weights;
    static constexpr int kNet = kNetNgp;
    static constexpr const char *kWho = "render_ngp_surface";
    static int check(const Weights *w) { return check_ngp_weights(w, kWho, true); }
    static NetPtrs ptrs(const Weights *w) { return ngp_ptrs(w); }
    static float bound(const Weights *w) { return w->bound; }
};
struct SirenSurf {
    using Weights = sdfr_siren_weights;
    static constexpr int kNet = kNetSiren;
    static constexpr const char *kWho = "render_siren_surface";
    static int check(const Weights *w) { return check_siren_weights(w, kWho, true); }
    static NetPtrs ptrs(const Weights *w) { return siren_ptrs(w); }
    static float bound(const Weights *) { return 0.0f; }
};

// What the evaluations of one surface call share: the network, the faces and the query
// sub-workspace with its FiLM vectors and weight region already prepared.
template <class SurfNet>
struct SurfEval {
    const typename SurfNet::Weights *w;
    NetPtrs P;
    uint32_t B;
    char *q;                       // the query sub-workspace
    const SurfWs *l;
    char *xws;                     // the packed weights' region
    hipStream_t st;
};

// The field at points [B,R,N,3] with the groups' directions dirs [B,R,3]: sdf [B,R,N] and,
// when rgb is non-null, the colour [B,R,N,3].  The SDF-only evaluations of the surface
// render (the coarse pass and every bisection step) pass rgb = nullptr and zero directions:
// the direction does not enter the SDF.
template <class SurfNet>
int sdf_at_points(const SurfEval<SurfNet> &e, uint32_t R, uint32_t N, const float *points,
                  const float *dirs, float *sdf, float *rgb) {
    int rc;
    if constexpr (SurfNet::kNet == kNetNgp) {
        const uint64_t S = (uint64_t)e.B * ((R + kTileRays - 1) / kTileRays) * N * kTileRays;
        float *enc = reinterpret_cast<float *>(e.q);
        const float *film = reinterpret_cast<const float *>(e.q + e.l->nq.film);
        f4 *gu = reinterpret_cast<f4 *>(e.q + e.l->nq.gu);
        const GeomArgs g = query_geom(e.B, R, N, S, dirs, e.w->bound);
        if ((rc = launch_query_geom(points, gu, g, e.st))) return rc;
        if ((rc = launch_encode(e.w, g, enc, gu, e.st))) return rc;
        return launch_qfield(kNetNgp, e.P, g, enc, e.xws, film, sdf, rgb, e.st);
    } else {
        const uint64_t S = siren_query_padded(e.B, R, N);
        const GeomArgs g = query_geom(e.B, R, N, S, dirs, 0.0f);
        return launch_qfield(kNetSiren, e.P, g, points, e.xws,
                             reinterpret_cast<const float *>(e.q), sdf, rgb, e.st);
    }
}

template <class SurfNet>
int surface_render(const typename SurfNet::Weights *w, const sdfr_surface_args *a,
                   hipStream_t st) {
    const char *who = SurfNet::kWho;
    if (!w || !a) return err(who, SDFR_EINVAL, "null args");
    if (a->B == 0 || a->H == 0 || a->W == 0 || a->N == 0)
        return err(who, SDFR_EINVAL, "empty batch / image / sample count");
    if (any_null({a->cam, a->focal, a->near_, a->far_, a->styles, a->pix_x, a->pix_y, a->t_vals,
                  a->workspace}))
        return err(who, SDFR_EINVAL, "required pointer is null");
    const bool want_grad = a->normal || a->residual;
    const bool maps = a->hit || a->sample || a->depth || a->xyz || a->rgb || want_grad;
    if (!a->sdf && !maps) return err(who, SDFR_EINVAL, "every output is null");
    if (a->refine_steps > 32) return err(who, SDFR_EINVAL, "refine_steps must be 0..32");
    int rc = SurfNet::check(w);                  // (the field kernel reads the colour head)
    if (rc) return rc;
    const SurfWs l = surf_ws(SurfNet::kNet, a->B, a->H, a->W, a->N);
    if (l.total == 0)
        return err(who, SDFR_EINVAL, "too many points per call (split the batch or the rows)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    char *ws = reinterpret_cast<char *>(a->workspace);
    auto at = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    const uint32_t B = a->B;
    SurfEval<SurfNet> e;
    e.w = w;
    e.P = SurfNet::ptrs(w);
    e.B = B;
    e.q = ws + l.q;
    e.l = &l;
    e.st = st;
    float *qfilm;
    if constexpr (SurfNet::kNet == kNetNgp) {
        e.xws = weight_region(a->prepacked, e.q + l.nq.x);
        qfilm = reinterpret_cast<float *>(e.q + l.nq.film);
    } else {
        e.xws = weight_region(a->prepacked, e.q + l.sq.x);
        qfilm = reinterpret_cast<float *>(e.q);
    }
    float *sdf = a->sdf ? a->sdf : at(l.sdf);
    float2 *zd = reinterpret_cast<float2 *>(ws + l.zd);
    f4 *br = reinterpret_cast<f4 *>(ws + l.br);
    int32_t *sidx = reinterpret_cast<int32_t *>(ws + l.sidx);
    float *dirs = at(l.dirs);
    const GeomArgs g = camera_geom(a, a->static_viewdirs, SurfNet::bound(w));

    // the coarse pass: the render's samples as H W groups of N points, zero directions
    if (hipMemsetAsync(dirs, 0, (size_t)B * l.M * 3 * sizeof(float), st) != hipSuccess)
        return err(who, SDFR_ELAUNCH, "zeroing the directions failed");
    if ((rc = launch_geom_points(g, at(l.pnet), zd, st))) return rc;
    if ((rc = launch_xprep(SurfNet::kNet, e.P, B, a->styles, e.xws, qfilm,
                           !a->prepacked, st)))
        return rc;
    if ((rc = sdf_at_points(e, l.M, a->N, at(l.pnet), dirs, sdf, nullptr))) return rc;
    if (!maps) return SDFR_OK;
    if ((rc = launch_surf_bracket(g, sdf, zd, br, sidx, st))) return rc;

    // K bisection steps on the H W midpoints per face, in groups of 32
    const float *f = nullptr;
    for (uint32_t k = 0; k < a->refine_steps; ++k) {
        if ((rc = launch_surf_step(g, l.Mp, f, br, at(l.pts), st))) return rc;
        if ((rc = sdf_at_points(e, l.Mp / 32, 32, at(l.pts), dirs, at(l.f), nullptr))) return rc;
        f = at(l.f);
    }
    if ((rc = launch_surf_hit(g, l.Mp, f, br, sidx, at(l.zs), at(l.hitp), dirs, st))) return rc;

    // the gradient and the colour at the hit points, each only when an output needs it
    if (want_grad) {
        char *gws = ws + l.g;
        if constexpr (SurfNet::kNet == kNetNgp) {
            if ((rc = ngp_gradient(w, B, l.M, at(l.hitp), a->styles, a->prepacked, gws, l.ng,
                                   at(l.gsdf), at(l.ggrad), st)))
                return rc;
        } else {
            float *gfilm = reinterpret_cast<float *>(gws);
            char *gx = weight_region(a->prepacked_grad, gws + l.sg.x);
            if ((rc = launch_gprep_siren(e.P, B, a->styles, gx, gfilm, !a->prepacked_grad, st)))
                return rc;
            if ((rc = launch_gfield(kNetSiren, e.P, gx, gfilm, at(l.hitp), at(l.gsdf),
                                    at(l.ggrad), B, l.M, 0.0f, st)))
                return rc;
        }
    }
    if (a->rgb &&
        (rc = sdf_at_points(e, l.M, 1, at(l.hitp), dirs, at(l.csdf), at(l.rgbq))))
        return rc;
    return launch_surf_maps(g, sidx, at(l.zs), at(l.gsdf), at(l.ggrad), at(l.rgbq), a->hit,
                            a->sample, a->depth, a->residual, a->xyz, a->normal, a->rgb, st);
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" {

// ----------------------------------------------------------------------------
// packing beforehand (once per weight version)
// ----------------------------------------------------------------------------
size_t sdfr_render_pack_bytes(int net) { return f16x3_ws_bytes(net); }

int sdfr_render_ngp_pack(const sdfr_ngp_weights *w, void *packed, void *stream) {
    if (!w || !packed) return fail(SDFR_EINVAL, "render_ngp_pack: null pointer");
    return launch_xprep(kNetNgp, ngp_ptrs(w), 0, nullptr, reinterpret_cast<char *>(packed),
                        nullptr, true, (hipStream_t)stream);
}

int sdfr_render_siren_pack(const sdfr_siren_weights *w, void *packed, void *stream) {
    if (!w || !packed) return fail(SDFR_EINVAL, "render_siren_pack: null pointer");
    return launch_xprep(kNetSiren, siren_ptrs(w), 0, nullptr, reinterpret_cast<char *>(packed),
                        nullptr, true, (hipStream_t)stream);
}

int sdfr_render_fc_pack(const sdfr_fc_weights *w, void *packed, void *stream) {
    if (!w || !packed) return fail(SDFR_EINVAL, "render_fc_pack: null pointer");
    return launch_xprep(kNetFc, fc_ptrs(w), 0, nullptr, reinterpret_cast<char *>(packed), nullptr,
                        true, (hipStream_t)stream);
}

size_t sdfr_query_siren_grad_pack_bytes(void) { return siren_grad_pack_bytes(); }

int sdfr_query_siren_grad_pack(const sdfr_siren_weights *w, void *packed, void *stream) {
    if (!w || !packed) return fail(SDFR_EINVAL, "query_siren_grad_pack: null pointer");
    if (int rc = check_siren_weights(w, "query_siren_grad_pack", false)) return rc;
    return launch_gprep_siren(siren_ptrs(w), 0, nullptr, reinterpret_cast<char *>(packed), nullptr,
                              true, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------
// render
// ----------------------------------------------------------------------------
size_t sdfr_render_ngp_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N,
                                       uint32_t num_levels) {
    return ngp_render_ws(B, H, W, N, num_levels).total;
}

int sdfr_render_ngp_encode_only(const sdfr_ngp_weights *w, const sdfr_ngp_render_args *a,
                                void *stream) {
    NgpRenderWs l;
    int rc = check_ngp_render(w, a, l);
    if (rc) return rc;
    const GeomArgs g = camera_geom(a, a->static_viewdirs, w->bound);
    char *ws = reinterpret_cast<char *>(a->workspace);
    f4 *gu = reinterpret_cast<f4 *>(ws + l.gu);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = launch_geom(g, nullptr, gu, st))) return rc;
    return launch_encode(w, g, reinterpret_cast<float *>(ws), gu, st);
}

int sdfr_render_ngp_forward(const sdfr_ngp_weights *w, const sdfr_ngp_render_args *a,
                            void *stream) {
    NgpRenderWs l;
    int rc = check_ngp_render(w, a, l);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *enc = reinterpret_cast<float *>(ws);
    float *film = reinterpret_cast<float *>(ws + l.film);
    f4 *gu = reinterpret_cast<f4 *>(ws + l.gu);
    const GeomArgs g = camera_geom(a, a->static_viewdirs, w->bound);
    record_event(a->stage_events[0], st);
    if (a->field_precision == SDFR_FIELD_F16X3) {
        // geometry and gather first (they do not read the styles), then the wait on
        // the caller's styles (ABI 11), the FiLM prep and the field kernel
        const NetPtrs P = ngp_ptrs(w);
        char *xws = weight_region(a->prepacked, ws + l.x);
        float2 *zd = reinterpret_cast<float2 *>(ws + l.zd);
        if ((rc = launch_geom(g, zd, gu, st))) return rc;
        record_event(a->stage_events[1], st);                  // the encode stage is the gather alone
        if ((rc = launch_encode(w, g, enc, gu, st))) return rc;
        record_event(a->stage_events[2], st);
        wait_event(a->styles_event, st);
        if ((rc = launch_xprep(kNetNgp, P, a->B, a->styles, xws, film, !a->prepacked, st)))
            return rc;
        record_event(a->field_event, st);
        float *part = reinterpret_cast<float *>(ws + l.part);
        if ((rc = launch_xfield(kNetNgp, P, a, g, enc, xws, film, st, part, zd))) return rc;
        record_event(a->stage_events[3], st);
        return SDFR_OK;
    }
    f4 *packed = reinterpret_cast<f4 *>(ws + l.packed);
    wait_event(a->styles_event, st);
    if ((rc = launch_prep(w, a, packed, film, st))) return rc;
    if ((rc = launch_geom(g, nullptr, gu, st))) return rc;
    record_event(a->stage_events[1], st);
    if ((rc = launch_encode(w, g, enc, gu, st))) return rc;
    record_event(a->stage_events[2], st);
    record_event(a->field_event, st);
    if ((rc = launch_field_fp32(w, a, g, enc, packed, film, st))) return rc;
    record_event(a->stage_events[3], st);
    return SDFR_OK;
}

size_t sdfr_render_siren_workspace_bytes(uint32_t B) {
    return f16x3_render_ws(kNetSiren, B, 0, 0, 0).total;
}

int sdfr_render_siren_forward(const sdfr_siren_weights *w, const sdfr_ngp_render_args *a,
                              void *stream) {
    const char *who = "render_siren";
    int rc = check_render_args(w, a, who, false);
    if (rc || (rc = check_siren_weights(w, who, true))) return rc;
    return render_f16x3(kNetSiren, who, siren_ptrs(w), a, (hipStream_t)stream);
}

size_t sdfr_render_fc_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    return f16x3_render_ws(kNetFc, B, H, W, N).total;
}

int sdfr_render_fc_forward(const sdfr_fc_weights *w, const sdfr_ngp_render_args *a, void *stream) {
    const char *who = "render_fc";
    int rc = check_render_args(w, a, who, false);
    if (rc || (rc = check_fc_weights(w, who))) return rc;
    return render_f16x3(kNetFc, who, fc_ptrs(w), a, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------
// field query at caller points (ABI 14): the render's gather (ngp) and f16x3 field stages
// with the points given instead of sampled along rays, and the per-sample SDF and colour
// stored instead of composited (kernels: field_query.hip)
// ----------------------------------------------------------------------------
size_t sdfr_query_ngp_workspace_bytes(uint32_t B, uint32_t R, uint32_t N) {
    return ngp_query_ws(B, R, N).total;
}

int sdfr_query_ngp_forward(const sdfr_ngp_weights *w, const sdfr_ngp_query_args *a,
                           void *stream) {
    const char *who = "query_ngp";
    int rc = check_query_args(w, a, who);
    if (rc || (rc = check_ngp_weights(w, who, true))) return rc;
    // the limit of the render (16 S < 2^32) and the field kernel's 32-bit byte offsets into
    // enc (128 S < 2^32); group and tile counts fit 32 bits below it
    const NgpQueryWs l = ngp_query_ws(a->B, a->R, a->N);
    if (l.S * 128 >= (1ull << 32) || (uint64_t)a->B * a->R >= (1ull << 32))
        return err(who, SDFR_EINVAL, "too many samples per call (split the points)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *enc = reinterpret_cast<float *>(ws);
    float *film = reinterpret_cast<float *>(ws + l.film);
    f4 *gu = reinterpret_cast<f4 *>(ws + l.gu);
    char *xws = weight_region(a->prepacked, ws + l.x);
    const NetPtrs P = ngp_ptrs(w);
    const GeomArgs g = query_geom(a->B, a->R, a->N, l.S, a->dirs, w->bound);
    if ((rc = launch_query_geom(a->points, gu, g, st))) return rc;
    if ((rc = launch_encode(w, g, enc, gu, st))) return rc;
    if ((rc = launch_xprep(kNetNgp, P, a->B, a->styles, xws, film, !a->prepacked, st))) return rc;
    return launch_qfield(kNetNgp, P, g, enc, xws, film, a->sdf, a->rgb, st);
}

size_t sdfr_query_siren_workspace_bytes(uint32_t B, uint32_t R, uint32_t N) {
    return siren_query_padded(B, R, N) ? f16x3_render_ws(kNetSiren, B, 0, 0, 0).total : 0;
}

int sdfr_query_siren_forward(const sdfr_siren_weights *w, const sdfr_siren_query_args *a,
                             void *stream) {
    const char *who = "query_siren";
    int rc = check_query_args(w, a, who);
    if (rc || (rc = check_siren_weights(w, who, true))) return rc;
    const uint64_t S = siren_query_padded(a->B, a->R, a->N);
    if (S == 0) return err(who, SDFR_EINVAL, "too many samples per call (split the points)");
    const FilmWs l = f16x3_render_ws(kNetSiren, a->B, 0, 0, 0);    // the render's workspace
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *film = reinterpret_cast<float *>(ws);
    char *xws = weight_region(a->prepacked, ws + l.x);
    const NetPtrs P = siren_ptrs(w);
    const GeomArgs g = query_geom(a->B, a->R, a->N, S, a->dirs, 0.0f);
    if ((rc = launch_xprep(kNetSiren, P, a->B, a->styles, xws, film, !a->prepacked, st)))
        return rc;
    return launch_qfield(kNetSiren, P, g, a->points, xws, film, a->sdf, a->rgb, st);
}

// ----------------------------------------------------------------------------
// SDF and its gradient at caller points (ABI 15): the gather with input derivatives (ngp)
// and the forward-mode f16x3 field kernel on the SDF trunk (kernels: field_grad.hip)
// ----------------------------------------------------------------------------
size_t sdfr_query_ngp_grad_workspace_bytes(uint32_t B, uint32_t M) {
    return ngp_grad_ws(B, M).total;
}

int sdfr_query_ngp_grad(const sdfr_ngp_weights *w, const sdfr_ngp_grad_args *a, void *stream) {
    const char *who = "query_ngp_grad";
    int rc = check_grad_args(w, a, who);
    if (rc || (rc = check_ngp_weights(w, who, false))) return rc;
    const NgpGradWs l = ngp_grad_ws(a->B, a->M);
    if (l.total == 0)
        return err(who, SDFR_EINVAL, "too many points per call (split the points)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    return ngp_gradient(w, a->B, a->M, a->points, a->styles, a->prepacked,
                        reinterpret_cast<char *>(a->workspace), l, a->sdf, a->grad,
                        (hipStream_t)stream);
}

size_t sdfr_query_siren_grad_workspace_bytes(uint32_t B, uint32_t M) {
    return siren_grad_ws(B, M).total;
}

int sdfr_query_siren_grad(const sdfr_siren_weights *w, const sdfr_siren_grad_args *a,
                          void *stream) {
    const char *who = "query_siren_grad";
    int rc = check_grad_args(w, a, who);
    if (rc || (rc = check_siren_weights(w, who, false))) return rc;
    const FilmWs l = siren_grad_ws(a->B, a->M);
    if (l.total == 0)
        return err(who, SDFR_EINVAL, "too many points per call (split the points)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *film = reinterpret_cast<float *>(ws);
    char *xws = weight_region(a->prepacked, ws + l.x);
    const NetPtrs P = siren_ptrs(w);
    if ((rc = launch_gprep_siren(P, a->B, a->styles, xws, film, !a->prepacked, st))) return rc;
    return launch_gfield(kNetSiren, P, xws, film, a->points, a->sdf, a->grad, a->B, a->M, 0.0f,
                         st);
}

// ----------------------------------------------------------------------------
// FC field query and SDF gradient at caller points: the FC render's FiLM prep and packing
// (launch_xprep), then field_r_kernel in query mode (field_fc_query.hip) or the forward-mode
// kernel on the first 116 slices of the same packing (field_grad.hip)
// ----------------------------------------------------------------------------
size_t sdfr_query_fc_workspace_bytes(uint32_t B, uint32_t R, uint32_t N) {
    return fc_query_ws(B, R, N).total;
}

int sdfr_query_fc_forward(const sdfr_fc_weights *w, const sdfr_fc_query_args *a, void *stream) {
    const char *who = "query_fc";
    int rc = check_query_args(w, a, who);
    if (rc || (rc = check_fc_weights(w, who))) return rc;
    const FilmWs l = fc_query_ws(a->B, a->R, a->N);
    if (l.total == 0)
        return err(who, SDFR_EINVAL, "too many samples per call (split the points)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *film = reinterpret_cast<float *>(ws);
    char *xws = weight_region(a->prepacked, ws + l.x);
    const NetPtrs P = fc_ptrs(w);
    const GeomArgs g = query_geom(a->B, a->R, a->N, siren_query_padded(a->B, a->R, a->N),
                                  a->dirs, 0.0f);
    if ((rc = launch_xprep(kNetFc, P, a->B, a->styles, xws, film, !a->prepacked, st))) return rc;
    return launch_qfield_fc(P, g, a->points, xws, film, a->sdf, a->rgb, st);
}

size_t sdfr_query_fc_grad_workspace_bytes(uint32_t B, uint32_t M) {
    return fc_grad_ws(B, M).total;
}

int sdfr_query_fc_grad(const sdfr_fc_weights *w, const sdfr_fc_grad_args *a, void *stream) {
    const char *who = "query_fc_grad";
    int rc = check_grad_args(w, a, who);
    if (rc || (rc = check_fc_weights(w, who))) return rc;
    const FilmWs l = fc_grad_ws(a->B, a->M);
    if (l.total == 0)
        return err(who, SDFR_EINVAL, "too many points per call (split the points)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *film = reinterpret_cast<float *>(ws);
    char *xws = weight_region(a->prepacked, ws + l.x);
    const NetPtrs P = fc_ptrs(w);
    if ((rc = launch_xprep(kNetFc, P, a->B, a->styles, xws, film, !a->prepacked, st))) return rc;
    return launch_gfield(kNetFc, P, xws, film, a->points, a->sdf, a->grad, a->B, a->M, 0.0f, st);
}

// ----------------------------------------------------------------------------
// Geometry render: the gradient call on the cameras' own samples, and normal / depth /
// xyz / mask maps composited with the render's weights (kernels: geometry.hip)
// ----------------------------------------------------------------------------
size_t sdfr_render_ngp_geometry_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    if (B == 0 || H == 0 || W == 0 || N == 0) return 0;
    return ngp_geom_ws(B, H, W, N).total;
}

int sdfr_render_ngp_geometry(const sdfr_ngp_weights *w, const sdfr_ngp_geometry_args *a,
                             void *stream) {
    const char *who = "render_ngp_geometry";
    if (!w || !a) return err(who, SDFR_EINVAL, "null args");
    if (a->B == 0 || a->H == 0 || a->W == 0 || a->N == 0)
        return err(who, SDFR_EINVAL, "empty batch / image / sample count");
    if (any_null({a->cam, a->focal, a->near_, a->far_, a->styles, a->pix_x, a->pix_y, a->t_vals,
                  a->workspace}))
        return err(who, SDFR_EINVAL, "required pointer is null");
    const bool composite = a->eikonal || a->normal || a->depth || a->xyz || a->mask;
    if (!a->sdf && !composite) return err(who, SDFR_EINVAL, "every output is null");
    int rc = check_ngp_weights(w, who, false);
    if (rc) return rc;
    if (!w->sigmoid_beta)
        return err(who, SDFR_EINVAL, "sigmoid_beta is required (no SDF, no gradient)");
    const NgpGeomWs l = ngp_geom_ws(a->B, a->H, a->W, a->N);
    if (l.total == 0)
        return err(who, SDFR_EINVAL, "too many points per call (split the batch or the rows)");
    if (a->workspace_bytes < l.total) return err(who, SDFR_EINVAL, "workspace too small");

    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(a->workspace);
    float *pnet = reinterpret_cast<float *>(ws + l.pnet);
    float2 *zd = reinterpret_cast<float2 *>(ws + l.zd);
    float *sdf = a->sdf ? a->sdf : reinterpret_cast<float *>(ws + l.sdf);
    float *gnet = reinterpret_cast<float *>(ws + l.gnet);
    const GeomArgs g = camera_geom(a, 0, w->bound);      // the network's view direction is not read
    if ((rc = launch_geom_points(g, pnet, zd, st))) return rc;
    if ((rc = ngp_gradient(w, a->B, l.M, pnet, a->styles, a->prepacked, ws, l.g, sdf, gnet, st)))
        return rc;
    if (!composite) return SDFR_OK;
    return launch_geom_composite(g, zd, sdf, gnet, w->sigmoid_beta, a->force_background,
                                 a->eikonal, a->normal, a->depth, a->xyz, a->mask, st);
}

// ----------------------------------------------------------------------------
// Surface render: per camera ray the SDF's first outside -> inside zero crossing, refined
// by bisection through the query call's kernels, with the normal (gradient call) and the
// colour (query call) there (ray-side kernels: surface.hip)
// ----------------------------------------------------------------------------
size_t sdfr_render_ngp_surface_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    return surf_ws(kNetNgp, B, H, W, N).total;
}

size_t sdfr_render_siren_surface_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t N) {
    return surf_ws(kNetSiren, B, H, W, N).total;
}

int sdfr_render_ngp_surface(const sdfr_ngp_weights *w, const sdfr_surface_args *a, void *stream) {
    return surface_render<NgpSurf>(w, a, (hipStream_t)stream);
}

int sdfr_render_siren_surface(const sdfr_siren_weights *w, const sdfr_surface_args *a,
                              void *stream) {
    return surface_render<SirenSurf>(w, a, (hipStream_t)stream);
}

}  // extern "C"

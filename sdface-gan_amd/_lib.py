"""ctypes binding of libsdfr.so (the C ABI declared in include/sdfr.h).

The library is built in-tree by ``make -C sdface-gan_amd`` (or
``__graft_entry__.build()``) into ``sdface-gan_amd/lib/libsdfr.so``.  There is
no fallback: if the library is missing or a call fails, a RuntimeError is
raised naming the entry point and the library's own message.
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("SDFR_LIB", PKG_DIR / "lib" / "libsdfr.so"))

_vp = ctypes.c_void_p
_u32 = ctypes.c_uint32
_f32 = ctypes.c_float
_int = ctypes.c_int

SDFR_OK = 0
SDFR_EINVAL = -1
SDFR_ELAUNCH = -2
SDFR_EUNSUPPORTED = -3
ABI_VERSION = 15
FIELD_F16X3 = 0
FIELD_FP32 = 1

class NgpWeights(ctypes.Structure):
    c_name = "sdfr_ngp_weights"
    _fields_ = [
        ("embeddings", _vp), ("offsets", _vp), ("num_levels", _u32),
        ("log2_per_level_scale", _f32), ("base_resolution", _u32), ("bound", _f32),
        ("input_w", _vp), ("input_b", _vp),
        ("pts_w", _vp * 3), ("pts_b", _vp * 3), ("pts_gw", _vp * 3), ("pts_gb", _vp * 3),
        ("pts_bw", _vp * 3), ("pts_bb", _vp * 3),
        ("views_w", _vp), ("views_b", _vp),
        ("views_gw", _vp), ("views_gb", _vp), ("views_bw", _vp), ("views_bb", _vp),
        ("sigma_w", _vp), ("sigma_b", _vp), ("rgb_w", _vp), ("rgb_b", _vp),
        ("sigmoid_beta", _vp),
    ]


class SirenWeights(ctypes.Structure):
    c_name = "sdfr_siren_weights"
    _fields_ = [
        ("depth", _u32), ("width", _u32),
        ("pts_w", _vp * 8), ("pts_b", _vp * 8), ("pts_gw", _vp * 8), ("pts_gb", _vp * 8),
        ("pts_bw", _vp * 8), ("pts_bb", _vp * 8),
        ("views_w", _vp), ("views_b", _vp),
        ("views_gw", _vp), ("views_gb", _vp), ("views_bw", _vp), ("views_bb", _vp),
        ("sigma_w", _vp), ("sigma_b", _vp), ("rgb_w", _vp), ("rgb_b", _vp),
        ("sigmoid_beta", _vp),
    ]


class FcWeights(ctypes.Structure):
    c_name = "sdfr_fc_weights"
    _fields_ = [
        ("depth", _u32), ("width", _u32),
        ("x_in_w", _vp), ("x_in_b", _vp), ("style_w", _vp), ("style_b", _vp),
        ("pts_w", _vp * 7), ("pts_b", _vp * 7),
        ("views_w", _vp), ("views_b", _vp),
        ("sigma_w", _vp), ("sigma_b", _vp), ("rgb_w", _vp), ("rgb_b", _vp),
        ("sigmoid_beta", _vp),
    ]


class NgpRenderArgs(ctypes.Structure):
    c_name = "sdfr_ngp_render_args"
    _fields_ = [
        ("B", _u32), ("H", _u32), ("W", _u32), ("N", _u32),
        ("cam", _vp), ("focal", _vp), ("near_", _vp), ("far_", _vp), ("styles", _vp),
        ("pix_x", _vp), ("pix_y", _vp), ("t_vals", _vp), ("t_rand", _vp), ("sigma_noise", _vp),
        ("t_rand_per_sample", _int), ("offset_sampling", _int), ("static_viewdirs", _int),
        ("z_normalize", _int), ("force_background", _int), ("with_sdf", _int),
        ("rgb", _vp), ("features", _vp), ("sdf", _vp), ("xyz", _vp), ("mask", _vp),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t),
        ("stage_events", _vp * 4), ("field_precision", _int), ("prepacked", _vp),
        ("max_field_segments", _u32),
        ("styles_event", _vp), ("field_event", _vp),
        ("features_split", _vp), ("features_mod", _vp),
    ]


class QueryArgs(ctypes.Structure):
    c_name = "sdfr_query_args"
    _fields_ = [
        ("B", _u32), ("R", _u32), ("N", _u32),
        ("points", _vp), ("dirs", _vp), ("styles", _vp), ("sdf", _vp), ("rgb", _vp),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("prepacked", _vp),
    ]


class GradArgs(ctypes.Structure):
    c_name = "sdfr_grad_args"
    _fields_ = [
        ("B", _u32), ("M", _u32),
        ("points", _vp), ("styles", _vp), ("sdf", _vp), ("grad", _vp),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("prepacked", _vp),
    ]


# the three networks' query / gradient calls take one struct each; the per-network names of
# the header's typedefs stay as aliases
NgpQueryArgs = SirenQueryArgs = FcQueryArgs = QueryArgs
NgpGradArgs = SirenGradArgs = FcGradArgs = GradArgs


class NgpGeometryArgs(ctypes.Structure):
    c_name = "sdfr_ngp_geometry_args"
    _fields_ = [
        ("B", _u32), ("H", _u32), ("W", _u32), ("N", _u32),
        ("cam", _vp), ("focal", _vp), ("near_", _vp), ("far_", _vp), ("styles", _vp),
        ("pix_x", _vp), ("pix_y", _vp), ("t_vals", _vp), ("t_rand", _vp),
        ("t_rand_per_sample", _int), ("offset_sampling", _int), ("z_normalize", _int),
        ("force_background", _int),
        ("sdf", _vp), ("eikonal", _vp), ("normal", _vp), ("depth", _vp), ("xyz", _vp),
        ("mask", _vp),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("prepacked", _vp),
    ]


class SurfaceArgs(ctypes.Structure):
    c_name = "sdfr_surface_args"
    _fields_ = [
        ("B", _u32), ("H", _u32), ("W", _u32), ("N", _u32),
        ("cam", _vp), ("focal", _vp), ("near_", _vp), ("far_", _vp), ("styles", _vp),
        ("pix_x", _vp), ("pix_y", _vp), ("t_vals", _vp), ("t_rand", _vp),
        ("t_rand_per_sample", _int), ("offset_sampling", _int), ("static_viewdirs", _int),
        ("z_normalize", _int), ("refine_steps", _u32),
        ("hit", _vp), ("sample", _vp), ("depth", _vp), ("residual", _vp),
        ("xyz", _vp), ("normal", _vp), ("rgb", _vp), ("sdf", _vp),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t),
        ("prepacked", _vp), ("prepacked_grad", _vp),
    ]


class RasterArgs(ctypes.Structure):
    c_name = "sdfr_raster_args"
    _fields_ = [
        ("B", _u32), ("H", _u32), ("W", _u32), ("V", _u32), ("F", _u32),
        ("vertices", _vp), ("faces", _vp), ("cam", _vp), ("focal", _vp),
        ("cx", _f32), ("cy", _f32), ("znear", _f32),
        ("face_idx", _vp), ("depth", _vp), ("bary", _vp),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t),
    ]


class StyledEpilogueArgs(ctypes.Structure):
    c_name = "sdfr_styled_epilogue_args"
    _fields_ = [
        ("B", _u32), ("C", _u32), ("H", _u32), ("W", _u32),
        ("conv", _vp), ("blur_up", _int), ("fir", _f32 * 4),
        ("demod", _vp), ("noise", _vp), ("noise_weight", _vp), ("bias", _vp),
        ("negative_slope", _f32), ("act_scale", _f32),
        ("s_next", _vp), ("y", _vp), ("rgb_w", _vp), ("rgb_b", _vp), ("skip", _vp), ("rgb", _vp),
        ("y_split", _vp),
    ]


class StyleArgs(ctypes.Structure):
    c_name = "sdfr_style_args"
    _fields_ = [
        ("B", _u32), ("n_latent", _u32), ("K", _u32), ("latent", _vp),
        ("L", _u32), ("cmax", _u32), ("mod_w", _vp), ("mod_b", _vp),
        ("mod_index", _u32 * 16), ("mod_c", _u32 * 16), ("mod_off", _u32 * 16), ("mods", _vp),
        ("J", _u32), ("omax", _u32), ("dem_w", _vp), ("dem_eps", _vp),
        ("dem_layer", _u32 * 16), ("dem_c", _u32 * 16), ("dem_off", _u32 * 16), ("demods", _vp),
    ]


class ConvActArgs(ctypes.Structure):
    c_name = "sdfr_conv_act_args"
    _fields_ = [
        ("x_split", _vp), ("packed", _vp),
        ("B", _u32), ("H", _u32), ("W", _u32), ("Cin", _u32), ("Cout", _u32),
        ("demod", _vp), ("noise", _vp), ("noise_weight", _vp), ("bias", _vp),
        ("negative_slope", _f32), ("act_scale", _f32),
        ("s_next", _vp), ("y_split", _vp), ("rgb_w", _vp), ("rgb_partial", _vp),
        ("ws", _vp), ("ws_bytes", ctypes.c_size_t),
        ("rgb_base", _vp), ("rgb_s", _vp),
    ]


class ConvTActArgs(ctypes.Structure):
    c_name = "sdfr_conv_t_act_args"
    _fields_ = [
        ("x_split", _vp), ("packed", _vp),
        ("B", _u32), ("H", _u32), ("W", _u32), ("Cin", _u32), ("Cout", _u32),
        ("fir", _f32 * 4),
        ("demod", _vp), ("noise", _vp), ("noise_weight", _vp), ("bias", _vp),
        ("negative_slope", _f32), ("act_scale", _f32),
        ("s_next", _vp), ("y_split", _vp), ("raw", _vp),
    ]


# sdfr_conv_plan: SDFR_CONV_EPI_* and the kernels named by SDFR_CONV_K_* (include/sdfr.h)
CONV_EPI_RAW, CONV_EPI_STYLED, CONV_EPI_BLUR = 0, 1, 2
CONV_PLAN_KERNELS = (
    "conv_x_kernel<false>", "conv_x_kernel<true>", "conv_splitk_kernel<false>",
    "conv_splitk_kernel<true>", "conv_h_kernel<false>", "conv_h_kernel<true>",
    "conv_h_finish_kernel", "conv_t_kernel<false>", "conv_t_kernel<true>",
    "conv_t_finish_kernel", "conv_t_border_kernel<true>", "conv_t_border_kernel<false>",
)


class ConvPlanQuery(ctypes.Structure):
    c_name = "sdfr_conv_plan_query"
    _fields_ = [
        ("B", _u32), ("H", _u32), ("W", _u32), ("Cin", _u32), ("Cout", _u32),
        ("transposed", _int), ("epilogue", _int), ("has_ws", _int),
        ("ws_bytes", ctypes.c_size_t),
    ]


class ConvPlanStep(ctypes.Structure):
    _fields_ = [("kernel", _u32), ("grid_x", _u32), ("grid_y", _u32), ("block", _u32)]


class ConvPlanInfo(ctypes.Structure):
    c_name = "sdfr_conv_plan_info"
    _fields_ = [
        ("rc", _int), ("ksplit", _u32), ("ksplit_t", _u32), ("ws_bytes", ctypes.c_size_t),
        ("nsteps", _u32), ("steps", ConvPlanStep * 6),
    ]


# ---------------------------------------------------------------------------
# The three renderer networks, each described once: the library's name for it (and its
# index, the ``kind`` / ``net`` of the Python and C side), its weights struct, and the
# struct's tensor members in the order of the flat tensor list that the registered op
# sdfr::render_fused takes (render_calls.weights_struct fills the struct by zipping the
# two).  sigmoid_beta is last (a placeholder tensor without an SDF).
# ---------------------------------------------------------------------------
Network = namedtuple("Network", ("name", "weights", "fields"))


def _layers(n, members):
    return tuple(f"pts_{m}[{l}]" for l in range(n) for m in members) + \
        tuple(f"views_{m}" for m in members)


_FILM = ("w", "b", "gw", "gb", "bw", "bb")      # a FiLM layer: w, b, gamma w, b, beta w, b
_HEADS = ("sigma_w", "sigma_b", "rgb_w", "rgb_b", "sigmoid_beta")
NETWORKS = (
    Network("ngp", NgpWeights, ("embeddings", "offsets", "input_w", "input_b")
            + _layers(3, _FILM) + _HEADS),
    Network("siren", SirenWeights, _layers(8, _FILM) + _HEADS),
    Network("fc", FcWeights, ("x_in_w", "x_in_b", "style_w", "style_b")
            + _layers(7, ("w", "b")) + _HEADS),
)

# ---------------------------------------------------------------------------
# Every function include/sdfr.h declares: name -> (restype, argtypes).  tests/test_abi.py
# compares the table with the header's prototypes and the structs above with its layouts.
# ---------------------------------------------------------------------------
_P = ctypes.POINTER
_sz = ctypes.c_size_t
_i64 = ctypes.c_int64
_GRID_BWD = [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _vp, _vp, _u32, _int,
             _u32]
_MC = [_vp, _u32, _u32, _u32, _i64, _i64, _i64, _f32, _vp, _sz]
_MC_SPARSE = [_vp, _vp, _vp, _u32, _u32, _f32, _vp, _sz, _vp]
PROTOTYPES = {
    "sdfr_abi_version": (_int, []),
    "sdfr_last_error": (ctypes.c_char_p, []),
    "sdfr_grid_encode_forward": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32,
                                        _vp, _u32, _int, _u32, _vp]),
    "sdfr_grid_encode_backward": (_int, _GRID_BWD + [_vp]),
    "sdfr_grid_encode_backward_ws_bytes": (_sz, [_u32, _u32, _u32, _u32, _f32, _u32, _int]),
    "sdfr_grid_encode_backward_ws": (_int, _GRID_BWD + [_vp, _sz, _vp]),
    "sdfr_sh_encode_forward": (_int, [_vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "sdfr_sh_encode_backward": (_int, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    # the three render workspaces depend on different sizes: prefixes of (B, H, W, N, levels)
    "sdfr_render_ngp_workspace_bytes": (_sz, [_u32] * 5),
    "sdfr_render_siren_workspace_bytes": (_sz, [_u32]),
    "sdfr_render_fc_workspace_bytes": (_sz, [_u32] * 4),
    "sdfr_render_pack_bytes": (_sz, [_int]),
    "sdfr_render_ngp_encode_only": (_int, [_P(NgpWeights), _P(NgpRenderArgs), _vp]),
    "sdfr_render_ngp_geometry_workspace_bytes": (_sz, [_u32] * 4),
    "sdfr_render_ngp_geometry": (_int, [_P(NgpWeights), _P(NgpGeometryArgs), _vp]),
    "sdfr_query_siren_grad_pack_bytes": (_sz, []),
    "sdfr_query_siren_grad_pack": (_int, [_P(SirenWeights), _vp, _vp]),
    "sdfr_debug_sin_probe": (_int, [_vp, _vp, _vp, _u32, _vp]),
    "sdfr_debug_sin_rev_probe": (_int, [_vp, _vp, _u32, _vp]),
    "sdfr_camera_extrinsics": (_int, [_vp, _vp, _u32, _f32, _f32, _f32] + [_vp] * 6),
    "sdfr_fused_bias_act": (_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _u32, _u32, _int, _int,
                                   _f32, _f32, _vp]),
    "sdfr_mapping_linear": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _f32, _f32, _int, _f32,
                                   _f32, _int, _vp]),
    "sdfr_decoder_styles": (_int, [_P(StyleArgs), _vp]),
    "sdfr_upfirdn2d": (_int, [_vp, _vp, _vp] + [_u32] * 5 + [_int] * 8 + [_vp]),
    "sdfr_styled_epilogue": (_int, [_P(StyledEpilogueArgs), _vp]),
    "sdfr_modulate_to_nhwc": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp]),
    "sdfr_modulate_to_nhwc_split": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp]),
    "sdfr_conv_pack_bytes": (_sz, [_u32, _u32]),
    "sdfr_conv_pack_weights": (_int, [_vp, _f32, _u32, _u32, _vp, _vp, _vp]),
    "sdfr_conv3x3_f16x3": (_int, [_vp, _vp, _vp] + [_u32] * 5 + [_int, _vp]),
    "sdfr_conv3x3_f16x3_ws": (_int, [_vp, _vp, _vp] + [_u32] * 5 + [_int, _vp, _sz, _vp]),
    "sdfr_conv_ws_bytes": (_sz, [_u32, _u32, _u32, _u32, _int]),
    "sdfr_set_conv_t_mode": (_int, [_int]),
    "sdfr_conv3x3_f16x3_act": (_int, [_P(ConvActArgs), _vp]),
    "sdfr_conv_t_act": (_int, [_P(ConvTActArgs), _vp]),
    "sdfr_conv_t_act_supported": (_int, [_u32] * 5),
    "sdfr_conv_act_ws_bytes": (_sz, [_u32] * 4),
    "sdfr_conv_plan": (_int, [_P(ConvPlanQuery), _P(ConvPlanInfo)]),
    "sdfr_rgb_finish": (_int, [_vp, _vp, _u32, _vp, _vp, _P(_f32), _u32, _u32, _u32, _vp]),
    "sdfr_mc_workspace_bytes": (_sz, [_u32] * 3),
    "sdfr_mc_count": (_int, _MC + [_P(_u32), _vp]),
    "sdfr_mc_emit": (_int, _MC + [_vp, _vp, _vp]),
    "sdfr_brick_layout_workspace_bytes": (_sz, [_u32]),
    "sdfr_brick_layout": (_int, [_vp, _u32, _vp, _u32, _vp, _sz, _P(_u32), _vp]),
    "sdfr_brick_points": (_int, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "sdfr_mc_sparse_workspace_bytes": (_sz, [_u32]),
    "sdfr_mc_sparse_count": (_int, _MC_SPARSE + [_P(_u32), _vp]),
    "sdfr_mc_sparse_emit": (_int, _MC_SPARSE + [_vp, _vp]),
    "sdfr_mesh_cc_workspace_bytes": (_sz, [_u32] * 2),
    "sdfr_mesh_cc_label": (_int, [_vp, _u32, _u32, _vp, _vp, _vp, _sz, _P(_u32), _vp]),
    "sdfr_mesh_cc_stats": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp,
                                  _P(ctypes.c_double), _vp, _sz, _vp]),
    "sdfr_mesh_cc_select_count": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _int, _vp, _sz,
                                         _P(_u32), _vp]),
    "sdfr_mesh_cc_select_emit": (_int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp,
                                        _vp, _vp]),
    "sdfr_mesh_simplify_workspace_bytes": (_sz, [_u32] * 2),
    "sdfr_mesh_simplify_count": (_int, [_vp, _vp, _u32, _u32, _f32, _f32, _f32, _f32, _u32, _u32,
                                        _u32, _int, _vp, _sz, _P(_u32), _vp]),
    "sdfr_mesh_simplify_emit": (_int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _vp,
                                       _vp, _vp, _vp]),
    "sdfr_mesh_smooth_workspace_bytes": (_sz, [_u32] * 2),
    "sdfr_mesh_smooth_prepare": (_int, [_vp, _vp, _u32, _u32, _f32, _f32, _f32, _int, _int, _vp,
                                        _sz, _vp, _vp, _vp]),
    "sdfr_mesh_smooth_run": (_int, [_vp, _u32, _P(_f32), _u32, _vp, _sz, _vp, _vp]),
    "sdfr_mesh_raster_workspace_bytes": (_sz, [_u32] * 5),
    "sdfr_mesh_raster": (_int, [_P(RasterArgs), _vp]),
    "sdfr_mesh_interpolate": (_int, [_vp, _u32, _u32, _vp, _u32, _vp, _vp, _u32, _u32, _u32,
                                     _vp, _u32, _f32, _vp, _vp]),
    "sdfr_linear_pack_bytes": (_sz, [_u32, _u32]),
    "sdfr_linear_pack": (_int, [_vp, _u32, _u32, _int, _vp, _vp]),
    "sdfr_linear_f16x3": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp]),
    "sdfr_linear_wgrad_ws_bytes": (_sz, [_u32] * 3),
    "sdfr_linear_wgrad_f16x3": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _sz, _vp]),
    "sdfr_film_linear_f16x3": (_int, [_vp] * 7 + [_u32] * 4 + [_vp]),
    "sdfr_film_backward_ws_bytes": (_sz, [_u32] * 3),
    "sdfr_film_backward": (_int, [_vp] * 8 + [_u32] * 3 + [_vp, _sz, _vp]),
    "sdfr_film_backward_grad_ws_bytes": (_sz, [_u32] * 3),
    "sdfr_film_backward_grad": (_int, [_vp] * 11 + [_u32] * 3 + [_vp, _sz, _vp]),
    "sdfr_linear_head_forward": (_int, [_vp] * 4 + [_u32] * 3 + [_vp]),
    "sdfr_linear_head_ws_bytes": (_sz, [_u32] * 3),
    "sdfr_linear_head_backward": (_int, [_vp] * 6 + [_u32] * 3 + [_vp, _sz, _vp]),
}
for _n in NETWORKS:
    _w = _P(_n.weights)
    PROTOTYPES.update({
        f"sdfr_render_{_n.name}_forward": (_int, [_w, _P(NgpRenderArgs), _vp]),
        f"sdfr_render_{_n.name}_pack": (_int, [_w, _vp, _vp]),
        f"sdfr_query_{_n.name}_workspace_bytes": (_sz, [_u32] * 3),
        f"sdfr_query_{_n.name}_forward": (_int, [_w, _P(QueryArgs), _vp]),
        f"sdfr_query_{_n.name}_grad_workspace_bytes": (_sz, [_u32] * 2),
        f"sdfr_query_{_n.name}_grad": (_int, [_w, _P(GradArgs), _vp]),
    })
    if _n.name != "fc":                         # (FC has the point calls only)
        PROTOTYPES.update({
            f"sdfr_render_{_n.name}_surface_workspace_bytes": (_sz, [_u32] * 4),
            f"sdfr_render_{_n.name}_surface": (_int, [_w, _P(SurfaceArgs), _vp]),
        })
# (tests check that the .so exports all of these and nothing else with the sdfr_ prefix)
EXPORTS = tuple(PROTOTYPES)

_lib = None


def lib():
    """Load libsdfr.so once; raise if it is absent (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"sdface-gan_amd: HIP library {LIB_PATH} is missing; build it with "
            "`make -C sdface-gan_amd` or `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    v = L.sdfr_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"libsdfr ABI {v} != expected {ABI_VERSION}; rebuild the library")
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != SDFR_OK:
        msg = lib().sdfr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_of(t):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

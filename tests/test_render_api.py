"""CPU: the argument checks of the three fused render calls (sdfr_render_{ngp,siren,fc}_forward)
and the values of every workspace / pack size function of the renderer (include/sdfr.h)."""
import ctypes

import pytest

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch

NETS = {
    "ngp": ("NgpWeights", "sdfr_render_ngp_forward", "sdfr_render_ngp_workspace_bytes"),
    "siren": ("SirenWeights", "sdfr_render_siren_forward", "sdfr_render_siren_workspace_bytes"),
    "fc": ("FcWeights", "sdfr_render_fc_forward", "sdfr_render_fc_workspace_bytes"),
}
REQUIRED = ("cam", "focal", "near_", "far_", "styles", "pix_x", "pix_y", "t_vals", "rgb",
            "workspace")


def _weights(sdfr, net):
    """The network's weight struct with every pointer non-null (never dereferenced on the
    host) and the shape the fused path takes."""
    w = getattr(sdfr._lib, NETS[net][0])()
    for name, typ in w._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, FAKE)
        elif hasattr(typ, "_length_"):
            setattr(w, name, typ(*([FAKE] * typ._length_)))
    if net == "ngp":
        w.num_levels, w.log2_per_level_scale, w.base_resolution, w.bound = 16, 0.5, 16, 1.0
    else:
        w.depth, w.width = 8, 256
    return w


def _ws_bytes(sdfr, net, a):
    fn = getattr(sdfr._lib.lib(), NETS[net][2])
    if net == "ngp":
        return fn(a.B, a.H, a.W, a.N, 16)
    return fn(a.B) if net == "siren" else fn(a.B, a.H, a.W, a.N)


def _args(sdfr, net, B=2, H=8, W=8, N=24):
    a = sdfr._lib.NgpRenderArgs(B=B, H=H, W=W, N=N, with_sdf=1)
    for name in REQUIRED:
        setattr(a, name, FAKE)
    a.workspace_bytes = _ws_bytes(sdfr, net, a)
    return a


def _rejected(sdfr, net, w, a, msg, code=None):
    lib = sdfr._lib.lib()
    rc = getattr(lib, NETS[net][1])(None if w is None else ctypes.byref(w),
                                    None if a is None else ctypes.byref(a), None)
    assert rc == (sdfr._lib.SDFR_EINVAL if code is None else code), (net, msg, rc)
    err = lib.sdfr_last_error()
    assert err.startswith(b"render_" + net.encode() + b": ") and msg in err, err


def _passes_to_next_check(sdfr, net, w, a):
    """The fields set so far are accepted: the last check of the call (the workspace size)
    answers, so nothing is launched."""
    a.workspace_bytes = _ws_bytes(sdfr, net, a) - 1
    _rejected(sdfr, net, w, a, b"workspace too small")


@pytest.mark.parametrize("net", sorted(NETS))
def test_render_rejects_bad_arguments_before_any_launch(sdfr, net):
    unsupported = sdfr._lib.SDFR_EUNSUPPORTED
    w = _weights(sdfr, net)
    _rejected(sdfr, net, None, _args(sdfr, net), b"null args")
    _rejected(sdfr, net, w, None, b"null args")
    for zero in ("B", "H", "W", "N"):
        a = _args(sdfr, net)
        setattr(a, zero, 0)
        _rejected(sdfr, net, w, a, b"empty batch / image / sample count")
    # field_precision: 0 = f16x3 (every network), 1 = fp32 (ngp only)
    a = _args(sdfr, net)
    a.field_precision = 1
    if net == "ngp":
        _passes_to_next_check(sdfr, net, w, a)
        a = _args(sdfr, net)
        a.field_precision = 2
        _rejected(sdfr, net, w, a, b"field_precision must be 0 (f16x3) or 1 (fp32)")
    else:
        _rejected(sdfr, net, w, a, b"only field_precision 0 (f16x3)", unsupported)
        a.field_precision = 2
        _rejected(sdfr, net, w, a, b"only field_precision 0 (f16x3)", unsupported)
    for bad in (3, 5, 8):
        a = _args(sdfr, net)
        a.max_field_segments = bad
        _rejected(sdfr, net, w, a, b"max_field_segments must be 0, 1, 2 or 4")
    for good in (0, 1, 2, 4):
        a = _args(sdfr, net)
        a.max_field_segments = good
        _passes_to_next_check(sdfr, net, w, a)
    for field in REQUIRED:
        a = _args(sdfr, net)
        setattr(a, field, None)
        _rejected(sdfr, net, w, a, b"required pointer is null")
    # weight pointers: the per-layer arrays (one entry null) and the single tensors
    for name, typ in w._fields_:
        w2 = _weights(sdfr, net)
        if hasattr(typ, "_length_"):
            n = typ._length_
            setattr(w2, name, typ(*([FAKE] * (n - 2) + [None, FAKE])))
            film = b"" if net == "fc" else b"FiLM "
            _rejected(sdfr, net, w2, _args(sdfr, net), film + b"weight pointer is null")
        elif typ is ctypes.c_void_p and name != "sigmoid_beta":
            setattr(w2, name, None)
            _rejected(sdfr, net, w2, _args(sdfr, net), b"weight pointer is null")
    # the network's shape
    if net == "ngp":
        for levels in (8, 15, 17):
            w2 = _weights(sdfr, net)
            w2.num_levels = levels
            _rejected(sdfr, net, w2, _args(sdfr, net), b"fused path needs 16 levels x 2 features",
                      unsupported)
    else:
        for field, value in (("depth", 7), ("depth", 9), ("width", 128), ("width", 512)):
            w2 = _weights(sdfr, net)
            setattr(w2, field, value)
            _rejected(sdfr, net, w2, _args(sdfr, net), b"fused path needs depth 8, width 256",
                      unsupported)
    # sigmoid_beta: read only when the network's output is an SDF
    w2 = _weights(sdfr, net)
    w2.sigmoid_beta = None
    _rejected(sdfr, net, w2, _args(sdfr, net), b"sigmoid_beta is required when with_sdf")
    a = _args(sdfr, net)
    a.with_sdf = 0
    _passes_to_next_check(sdfr, net, w2, a)
    # the workspace
    a = _args(sdfr, net)
    a.workspace_bytes -= 1
    _rejected(sdfr, net, w, a, b"workspace too small")
    a.workspace_bytes = 0
    _rejected(sdfr, net, w, a, b"workspace too small")
    # every optional field set is accepted
    a = _args(sdfr, net)
    for field in ("t_rand", "sigma_noise", "features", "sdf", "xyz", "mask", "prepacked"):
        setattr(a, field, FAKE)
    _passes_to_next_check(sdfr, net, w, a)


def test_render_ngp_rejects_features_split_misuse(sdfr):
    w = _weights(sdfr, "ngp")
    a = _args(sdfr, "ngp")
    a.features_split, a.features_mod, a.field_precision = FAKE, FAKE, 1
    _rejected(sdfr, "ngp", w, a, b"features_split needs the f16x3 field",
              sdfr._lib.SDFR_EUNSUPPORTED)
    a = _args(sdfr, "ngp")
    a.features_split = FAKE                                 # no features_mod
    _rejected(sdfr, "ngp", w, a, b"features_split takes features_mod and no features")
    a.features_mod, a.features = FAKE, FAKE                 # NCHW features beside it
    _rejected(sdfr, "ngp", w, a, b"features_split takes features_mod and no features")
    a.features = None
    _passes_to_next_check(sdfr, "ngp", w, a)
    # the sample limit of one call (16 S < 2^32) is the last check
    a = _args(sdfr, "ngp", B=1 << 12, H=1 << 8, W=1 << 8, N=1)
    _rejected(sdfr, "ngp", w, a, b"too many samples per call")


# Every size function at fixed shapes.  B = 1, 2 and 32 at 64 x 64 x 24 give 4, 2 and 1
# sample segments of the partials region (ngp and FC renders); R and M go through the
# padding units 8 and 16; the point limits (2^25 padded points for the ngp gradient and the
# geometry render, 2^30 for the SIREN calls, which answer 0 from the limit on; 128 S < 2^32
# for the ngp query, whose size function has no limit of its own) appear with the first
# size on each side.
PINNED = {
    "sdfr_render_ngp_workspace_bytes": {
        (1, 64, 64, 24, 16): 34227200,
        (2, 64, 64, 24, 16): 49177600,
        (32, 64, 64, 24, 16): 480388096,
        (1, 8, 8, 24, 16): 2487296,
        (2, 7, 9, 5, 16): 2359296,
        (3, 13, 11, 24, 16): 5400576,
        (2, 8, 8, 24, 8): 2802688,
    },
    "sdfr_render_siren_workspace_bytes": {
        (1,): 2199552,
        (2,): 2217984,
        (32,): 2770944,
        (0,): 2181120,
    },
    "sdfr_render_fc_workspace_bytes": {
        (1, 64, 64, 24): 19533824,
        (2, 64, 64, 24): 19552256,
        (32, 64, 64, 24): 2803712,
        (2, 8, 8, 24): 2791424,
        (3, 13, 11, 5): 3181568,
    },
    "sdfr_render_pack_bytes": {
        (0,): 877568,
        (1,): 2181120,
        (2,): 2213888,
    },
    "sdfr_query_siren_grad_pack_bytes": {
        (): 1867776,
    },
    "sdfr_query_ngp_workspace_bytes": {
        (1, 16, 32): 959488,
        (2, 7, 3): 907776,
        (2, 8, 3): 907776,
        (2, 9, 3): 907776,
        (2, 15, 3): 907776,
        (2, 16, 3): 907776,
        (2, 17, 3): 921600,
        (2, 41, 1): 907776,
        (1, 2097136, 16): 4832687104,
        (1, 2097137, 16): 4832723968,
        (1, 2097152, 16): 4832723968,
    },
    "sdfr_query_ngp_grad_workspace_bytes": {
        (1, 40): 906240,
        (2, 7): 902144,
        (2, 8): 902144,
        (2, 9): 910336,
        (2, 15): 910336,
        (2, 16): 910336,
        (2, 17): 918528,
        (2, 41): 943104,
        (1, 33554424): 17180750848,
        (1, 33554425): 0,
        (1, 33554432): 0,
        (4, 8388608): 0,
        (4, 8388600): 17180763136,
        (0, 8): 877568,
        (1, 0): 885760,
    },
    "sdfr_render_ngp_geometry_workspace_bytes": {
        (1, 64, 64, 24): 54756352,
        (2, 64, 64, 24): 108635136,
        (32, 64, 64, 24): 1724998656,
        (2, 8, 8, 24): 2577408,
        (2, 7, 9, 5): 1244672,
        (3, 13, 11, 3): 1612800,
        (1, 2048, 2047, 8): 18379736064,
        (1, 2048, 2048, 8): 0,
        (2, 2048, 1024, 8): 0,
        (1, 1, 33554424, 1): 18388710400,
        (1, 1, 33554425, 1): 0,
        (0, 8, 8, 24): 0,
    },
    "sdfr_query_siren_workspace_bytes": {
        (1, 3, 32): 2199552,
        (2, 7, 3): 2217984,
        (2, 8, 3): 2217984,
        (2, 9, 3): 2217984,
        (2, 15, 3): 2217984,
        (2, 16, 3): 2217984,
        (2, 17, 3): 2217984,
        (2, 41, 1): 2217984,
        (32, 16, 4): 2770944,
        (1, 67108848, 16): 2199552,
        (1, 67108849, 16): 0,
        (0, 3, 32): 0,
    },
    "sdfr_query_siren_grad_workspace_bytes": {
        (1, 40): 1884160,
        (2, 7): 1900544,
        (2, 8): 1900544,
        (2, 9): 1900544,
        (2, 15): 1900544,
        (2, 16): 1900544,
        (2, 17): 1900544,
        (2, 41): 1900544,
        (32, 64): 2392064,
        (1, 1073741816): 1884160,
        (1, 1073741817): 0,
        (0, 40): 0,
        (1, 0): 0,
    },
}


@pytest.mark.parametrize("fn", sorted(PINNED))
def test_workspace_and_pack_sizes_are_pinned(sdfr, fn):
    f = getattr(sdfr._lib.lib(), fn)
    got = {shape: f(*shape) for shape in PINNED[fn]}
    assert got == PINNED[fn]

"""CPU: the SIREN field query's and SDF gradient's C-ABI argument checks and workspace
sizes (sdfr_query_siren_forward, sdfr_query_siren_grad, include/sdfr.h), and
VolumeFeatureRenderer.query / query_gradient on a CPU SIREN renderer (the module path)."""
import ctypes

import pytest
import torch

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch
LIMIT = 1 << 30        # padded points per call: the first rejected count (include/sdfr.h)


def _weights(sdfr):
    """sdfr_siren_weights with every pointer non-null (never dereferenced on the host)."""
    w = sdfr._lib.SirenWeights()
    for name, typ in w._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, FAKE)
        elif typ is not ctypes.c_uint32:
            setattr(w, name, typ(*([FAKE] * 8)))
    w.depth, w.width = 8, 256
    return w


def _qargs(sdfr, B=1, R=3, N=32):
    lib = sdfr._lib.lib()
    return sdfr._lib.SirenQueryArgs(
        B=B, R=R, N=N, points=FAKE, dirs=FAKE, styles=FAKE, sdf=FAKE, rgb=None, workspace=FAKE,
        workspace_bytes=lib.sdfr_query_siren_workspace_bytes(B, R, N), prepacked=None)


def _gargs(sdfr, B=1, M=40):
    lib = sdfr._lib.lib()
    return sdfr._lib.SirenGradArgs(
        B=B, M=M, points=FAKE, styles=FAKE, sdf=None, grad=FAKE, workspace=FAKE,
        workspace_bytes=lib.sdfr_query_siren_grad_workspace_bytes(B, M), prepacked=None)


def _rejected(sdfr, fn, w, a, msg, code=None):
    lib = sdfr._lib.lib()
    rc = getattr(lib, fn)(None if w is None else ctypes.byref(w),
                          None if a is None else ctypes.byref(a), None)
    assert rc == (sdfr._lib.SDFR_EINVAL if code is None else code), (fn, msg, rc)
    err = lib.sdfr_last_error()
    prefix = b"query_siren_grad: " if fn.endswith("grad") else b"query_siren: "
    assert err.startswith(prefix) and msg in err, err


def _weight_rejections(sdfr, fn, args, colour):
    w = _weights(sdfr)
    _rejected(sdfr, fn, None, args(sdfr), b"null args")
    _rejected(sdfr, fn, w, None, b"null args")
    for name in ("pts_w", "pts_b", "pts_gw", "pts_gb", "pts_bw", "pts_bb"):
        w2 = _weights(sdfr)
        setattr(w2, name, (ctypes.c_void_p * 8)(*([FAKE] * 5 + [None] + [FAKE] * 2)))
        _rejected(sdfr, fn, w2, args(sdfr), b"FiLM weight pointer is null")
    for name in ("sigma_w", "sigma_b"):
        w2 = _weights(sdfr)
        setattr(w2, name, None)
        _rejected(sdfr, fn, w2, args(sdfr), b"weight pointer is null")
    for name in ("views_w", "views_b", "views_gw", "views_gb", "views_bw", "views_bb", "rgb_w",
                 "rgb_b"):
        w2 = _weights(sdfr)
        setattr(w2, name, None)
        if colour:
            _rejected(sdfr, fn, w2, args(sdfr), b"weight pointer is null")
        else:
            # the gradient does not read the colour layers: the next check answers
            a = args(sdfr)
            a.workspace_bytes = 0
            _rejected(sdfr, fn, w2, a, b"workspace too small")
    for field, value in (("depth", 7), ("width", 128)):
        w2 = _weights(sdfr)
        setattr(w2, field, value)
        _rejected(sdfr, fn, w2, args(sdfr), b"needs depth 8, width 256",
                  sdfr._lib.SDFR_EUNSUPPORTED)


def test_siren_query_rejects_bad_arguments_before_any_launch(sdfr):
    fn, w = "sdfr_query_siren_forward", _weights(sdfr)
    _weight_rejections(sdfr, fn, _qargs, colour=True)
    for zero in ("B", "R", "N"):
        a = _qargs(sdfr)
        setattr(a, zero, 0)
        _rejected(sdfr, fn, w, a, b"empty batch / group / point count")
    for field in ("points", "dirs", "styles", "sdf", "workspace"):
        a = _qargs(sdfr)
        setattr(a, field, None)
        _rejected(sdfr, fn, w, a, b"required pointer is null")
    a = _qargs(sdfr)
    a.rgb = None                                            # optional: the next check answers
    a.workspace_bytes -= 1
    _rejected(sdfr, fn, w, a, b"workspace too small")
    a.workspace_bytes = 0
    _rejected(sdfr, fn, w, a, b"workspace too small")
    # 2^30 padded points B x (R rounded up to 16) x N are the first rejected size; one
    # padding unit below passes that check and reaches the next one
    a = _qargs(sdfr, B=1, R=(1 << 26) - 15, N=16)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, fn, w, a, b"too many samples per call")
    a = _qargs(sdfr, B=1, R=(1 << 26) - 16, N=16)
    a.workspace_bytes = 0
    _rejected(sdfr, fn, w, a, b"workspace too small")
    a = _qargs(sdfr, B=4, R=1 << 20, N=256)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, fn, w, a, b"too many samples per call")
    # products that wrap in 32 or 64 bits
    for B, R, N in (((1 << 32) - 1,) * 3, (1 << 31, 1, 1 << 26), (1, 1 << 31, 2),
                    (3, (1 << 32) - 1, (1 << 32) - 1), (1 << 16, 1 << 16, 1 << 31),
                    (1, (1 << 32) - 1, 1), (1 << 30, 16, 4)):
        a = _qargs(sdfr, B=B, R=R, N=N)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, fn, w, a, b"too many samples per call")
        a.workspace_bytes = 0
        _rejected(sdfr, fn, w, a, b"too many samples per call")


def test_siren_gradient_rejects_bad_arguments_before_any_launch(sdfr):
    fn, w = "sdfr_query_siren_grad", _weights(sdfr)
    _weight_rejections(sdfr, fn, _gargs, colour=False)
    for zero in ("B", "M"):
        a = _gargs(sdfr)
        setattr(a, zero, 0)
        _rejected(sdfr, fn, w, a, b"empty batch / point count")
    for field in ("points", "styles", "grad", "workspace"):
        a = _gargs(sdfr)
        setattr(a, field, None)
        _rejected(sdfr, fn, w, a, b"required pointer is null")
    a = _gargs(sdfr)
    a.workspace_bytes -= 1
    _rejected(sdfr, fn, w, a, b"workspace too small")
    a.workspace_bytes = 0
    _rejected(sdfr, fn, w, a, b"workspace too small")
    # 2^30 padded points (M rounded up to 8 per face) are the first rejected size
    a = _gargs(sdfr, B=1, M=LIMIT - 7)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, fn, w, a, b"too many points per call")
    a = _gargs(sdfr, B=1, M=LIMIT - 8)
    a.workspace_bytes = 0
    _rejected(sdfr, fn, w, a, b"workspace too small")
    a = _gargs(sdfr, B=4, M=1 << 28)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, fn, w, a, b"too many points per call")
    # sizes whose 32-bit (3 x point index) or 64-bit products would wrap
    for B, M in (((1 << 32) - 1, (1 << 32) - 1), (1 << 26, 1 << 31), (1 << 23, (1 << 32) - 1),
                 (1 << 31, 1 << 26), (1, (1 << 32) - 1), (1 << 31, 2)):
        a = _gargs(sdfr, B=B, M=M)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, fn, w, a, b"too many points per call")
        a.workspace_bytes = 0
        _rejected(sdfr, fn, w, a, b"too many points per call")
    # the packing call
    lib = sdfr._lib.lib()
    assert lib.sdfr_query_siren_grad_pack(None, FAKE, None) == sdfr._lib.SDFR_EINVAL
    assert lib.sdfr_query_siren_grad_pack(ctypes.byref(w), None, None) == sdfr._lib.SDFR_EINVAL
    assert b"query_siren_grad_pack" in lib.sdfr_last_error()
    w2 = _weights(sdfr)
    w2.depth = 4
    assert lib.sdfr_query_siren_grad_pack(ctypes.byref(w2), FAKE, None) == \
        sdfr._lib.SDFR_EUNSUPPORTED


def test_siren_workspace_size_functions(sdfr):
    """Both workspaces hold per-face FiLM vectors and a weight-packing region and do not
    grow with the points; 0 for zero sizes and for sizes at or beyond the point limit."""
    lib = sdfr._lib.lib()
    q, g = lib.sdfr_query_siren_workspace_bytes, lib.sdfr_query_siren_grad_workspace_bytes
    pack_r, pack_g = lib.sdfr_render_pack_bytes(1), lib.sdfr_query_siren_grad_pack_bytes()
    # the trunk in one slice of 16 KiB per k-step of 16 K (1 + 7 x 16) + row scales and
    # scaled biases of 8 layers
    assert pack_g == 113 * 16384 + 2 * 8 * 256 * 4
    assert q(0, 3, 32) == q(1, 0, 32) == q(1, 3, 0) == 0
    assert g(0, 40) == g(1, 0) == 0
    # query: 9 FiLM sets per face (gamma, beta x 256 fp32), then the render's packing
    assert q(1, 3, 32) >= 9 * 2 * 256 * 4 + pack_r
    assert q(2, 3, 32) == q(1, 3, 32) + 9 * 2 * 256 * 4
    assert g(1, 40) >= 8 * 2 * 256 * 4 + pack_g
    assert g(2, 40) == g(1, 40) + 8 * 2 * 256 * 4
    # equal within a padding unit (16 groups / 8 points), non-decreasing in each argument
    assert q(1, 1, 32) == q(1, 16, 32) == q(1, 17, 32)
    assert g(1, 1) == g(1, 7) == g(1, 8) == g(1, 9)
    sizes = [q(b, r, n) for b in (1, 2, 5) for r in (1, 16, 17, 400) for n in (1, 3, 32)]
    assert all(s > 0 for s in sizes)
    for b in (1, 2, 5):
        assert q(b, 16, 4) <= q(b + 1, 16, 4) and q(b, 16, 4) <= q(b, 17, 4) <= q(b, 17, 5)
        assert g(b, 64) <= g(b + 1, 64) and g(b, 64) <= g(b, 65)
    # the point limit: positive one padding unit below, 0 at and beyond it
    assert q(1, (1 << 26) - 16, 16) == q(1, 1, 1) > 0
    assert q(1, (1 << 26) - 15, 16) == 0 == q(1, 1 << 26, 16) == q(1, 16, 1 << 26)
    assert q(1 << 26, 16, 1) == 0 and q((1 << 26) - 1, 16, 1) > 0
    assert q((1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1) == 0 == q(1 << 31, 1, 1 << 26)
    assert g(1, LIMIT - 8) == g(1, 1) > 0
    assert g(1, LIMIT - 7) == 0 == g(1, LIMIT) == g(1 << 26, 1 << 31)
    assert g((1 << 32) - 1, (1 << 32) - 1) == 0 == g(1 << 27, 8) and g((1 << 27) - 1, 8) > 0


def test_query_on_a_cpu_siren_renderer_is_the_module_path(sdfr):
    """Unchanged behaviour: on CPU tensors a SIREN renderer's query / query_gradient are the
    network evaluated op by op, exactly; encode_only is the ngp gather's and raises."""
    opt = sdfr.vol_render_opt(ngp=False)
    torch.manual_seed(4)
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=8).eval()
    assert ren._net_kind() == 1
    B, M = 2, 5
    pts = torch.rand(B, M, 3) * 2 - 1
    lat = torch.randn(B, 256)
    dirs = torch.nn.functional.normalize(torch.randn(B, M, 3), dim=-1)
    assert not ren._query_fused_ok(pts, lat)
    with torch.no_grad():
        raw = ren.network(torch.cat([pts, dirs], -1), styles=lat)
        sdf, rgb = ren.query(pts, lat, viewdirs=dirs)
        raw1 = ren.network(torch.cat([pts, dirs[:, :1].expand(B, M, 3)], -1), styles=lat)
        sdf1, rgb1 = ren.query(pts, lat, viewdirs=dirs[:, 0])
        sdf0, none = ren.query(pts, lat, return_rgb=False)
    assert torch.equal(sdf, raw[..., 3]) and torch.equal(rgb, torch.sigmoid(raw[..., :3]))
    assert torch.equal(sdf1, raw1[..., 3]) and torch.equal(rgb1, torch.sigmoid(raw1[..., :3]))
    assert none is None and torch.equal(sdf0, sdf)          # the SDF ignores the direction
    p = pts.clone().requires_grad_(True)
    out = ren.network(torch.cat([p, torch.zeros(B, M, 3)], -1), styles=lat)
    want, = torch.autograd.grad(out[..., 3].sum(), p)
    assert want.abs().max() > 0
    with torch.no_grad():
        gs, grad = ren.query_gradient(pts, lat)
    assert torch.equal(grad, want) and torch.equal(gs, out[..., 3].detach())
    assert not grad.requires_grad and not pts.requires_grad
    with pytest.raises(ValueError, match="encode_only"):
        ren.query_gradient(pts, lat, encode_only=True)

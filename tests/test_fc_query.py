"""CPU: the FC field query's and SDF gradient's C-ABI exports, argument checks and workspace
sizes (sdfr_query_fc_forward, sdfr_query_fc_grad, include/sdfr.h), and the float64
reference of the FC accuracy tests (shared with tests/test_gpu_fc_query.py), checked on
the CPU against the fp32 module itself."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch
LIMIT = 1 << 30        # padded points per call: the first rejected count (include/sdfr.h)
FILM = 9 * 2 * 256 * 4     # one face's FiLM slots: 9 layers x (1/su, bias) x 256 fp32

# A point is left out of a gradient comparison when, in the float64 reference, a
# pre-activation of any layer lies within KINK of that layer's largest magnitude over the
# batch: the gradient of a ReLU network jumps where a pre-activation changes sign, so there
# fp32 and float64 may stand on different linear pieces (a flipped mask moves the gradient
# by percents of its size; rounding by 1e-6 of it).  The share left out stays below
# MAX_LEFT_OUT.
KINK = 1e-5
MAX_LEFT_OUT = 0.10
# of max |grad| over the batch: no kept point of an fp32 evaluation is further from the
# reference (rounding sits near 1e-6, a flipped mask at 1.6e-2 and above)
POINT_MAX = 1e-3
# mean error of the fp32 module on the kept points, of max |grad|
MODULE_MEAN = 1e-6


# ---------------------------------------------------------------------------- reference
def alive_renderer(sdfr):
    """Set (a): a seeded FC renderer with every pts_linears weight doubled, so that all
    eight layers shape the SDF (the golden FC weights are dead beyond layer 2: one
    activation pattern at layer 7 and |grad| <= 1e-8)."""
    torch.manual_seed(3)
    ren = sdfr.VolumeFeatureRenderer(sdfr.vol_render_opt(ngp=False, fc=True).rendering,
                                     style_dim=256, out_im_res=8).eval()
    with torch.no_grad():
        for layer in ren.network.pts_linears:
            layer.weight *= 2
    return ren


def alive_inputs():
    """Set (a)'s points [2,4096,3] in [-1,1]^3 and styles [2,256]."""
    gen = torch.Generator().manual_seed(1)
    pts = torch.rand(2, 4096, 3, generator=gen) * 2 - 1
    return pts, torch.randn(2, 256, generator=gen)


def _enc64(p, L, tangent):
    """FCGenerator.transform_points in float64 with the fp32 module's own arguments:
    arg = fp32(fp32(2^i pi) fp32(p / 2)), and (tangent) the slope c_i / 2 with respect to
    p.  A plain float64 encoding would differ from the fp32 module by the rounding of the
    argument alone (3.4e-5 of max |grad|), the same term in both arms of a comparison."""
    p32 = p.detach().float()
    half = p32 / 2
    parts = []
    for i in range(L):
        c = torch.tensor((2 ** i) * np.pi, dtype=torch.float32)
        arg = (c * half).double()
        if tangent:
            arg = arg + (c.double() / 2) * (p - p.detach())
        parts.append(torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1))
    return torch.cat(parts, dim=-1)


def ref64(ren, pts, dirs, lat):
    """The float64 reference of renderer ``ren``'s FC network at fp32 ``pts`` [B,M,3] with
    view directions ``dirs`` ([B,M,3], [B,3] or None: zeros) and styles ``lat``: dict of
    numpy sdf [B,M], rgb [B,M,3] in [0,1], grad [B,M,3] and keep [B,M] (the kink rule)."""
    net = copy.deepcopy(ren.network).cpu().double()
    p = torch.as_tensor(pts).detach().cpu().float().double().requires_grad_(True)
    B, M = p.shape[:2]
    d = torch.zeros(B, M, 3) if dirs is None else torch.as_tensor(dirs).detach().cpu().float()
    d = d if d.dim() == 3 else d.unsqueeze(1).expand(B, M, 3)
    s = net.style_in(torch.as_tensor(lat).detach().cpu().double()).unsqueeze(1)
    pre = net.x_in(_enc64(p, net.n_freq_posenc, True)) + s
    keep = torch.ones(B, M, dtype=torch.bool)
    layers = list(net.pts_linears)
    for k in range(len(layers) + 1):
        keep &= (pre.detach().abs() >= KINK * pre.detach().abs().max()).all(-1)
        h = F.relu(pre)
        if k < len(layers):
            pre = layers[k](h)
    sdf = net.sigma_linear(h)[..., 0]
    grad, = torch.autograd.grad(sdf.sum(), p)
    with torch.no_grad():
        views = _enc64(d.double(), net.n_freq_posenc_views, False)
        rgb = torch.sigmoid(net.rgb_linear(net.views_linears(torch.cat([h, views], -1))))
    return dict(sdf=sdf.detach().numpy(), rgb=rgb.numpy(), grad=grad.numpy(),
                keep=keep.numpy())


def point_err(grad, ref):
    """Per point, |grad - ref| (Euclidean) of max |ref| over the batch."""
    ref = np.asarray(ref, np.float64)
    err = np.linalg.norm(np.asarray(grad, np.float64) - ref, axis=-1)
    return err / np.linalg.norm(ref, axis=-1).max()


def module_grad(ren, pts, lat):
    """(sdf, grad) of the op-by-op fp32 path: autograd through renderer.network."""
    p = pts.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        raw = ren.network(torch.cat([p, torch.zeros_like(p)], -1), styles=lat.detach())
        g, = torch.autograd.grad(raw[..., 3].sum(), p)
    return raw[..., 3].detach().cpu().numpy(), g.cpu().numpy()


@pytest.fixture(scope="module")
def alive(sdfr):
    ren = alive_renderer(sdfr)
    pts, lat = alive_inputs()
    return ren, pts, lat, ref64(ren, pts, None, lat)


def test_reference_keeps_most_points_and_the_fp32_module_meets_it(alive):
    """The float64 reference on set (a): it is alive (gradients of order 10), the kink rule
    leaves out at most 10 % of the points, and on the kept points the fp32 module is at
    rounding distance -- mean <= 1e-6 of max |grad|, no point above 1e-3."""
    ren, pts, lat, ref = alive
    norm = np.linalg.norm(ref["grad"], axis=-1)
    left_out = 1.0 - float(ref["keep"].mean())
    sdf, grad = module_grad(ren, pts, lat)
    err = point_err(grad, ref["grad"])
    kept = err[ref["keep"]]
    print(f"set (a): |grad| max {norm.max():.3g} median {np.median(norm):.3g}; left out "
          f"{left_out:.4f}; fp32 module on kept points: mean {kept.mean():.3e} max "
          f"{kept.max():.3e}; on all points max {err.max():.3e}")
    assert norm.max() > 1.0 and np.median(norm) > 0.1
    assert left_out <= MAX_LEFT_OUT
    assert kept.mean() <= MODULE_MEAN and kept.max() <= POINT_MAX


def test_reference_slope_is_the_derivative_of_its_own_encoding():
    """The tangent the reference gives autograd is c_i / 2 times cos / -sin of the fp32
    argument: what the gradient kernel's layer-0 tangent columns hold."""
    p = (torch.rand(1, 7, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).double()
    p.requires_grad_(True)
    enc = _enc64(p, 10, True)
    assert enc.shape == (1, 7, 60)
    half = p.detach().float() / 2
    for e in (0, 4, 29, 57):
        i, r = divmod(e, 6)
        c = torch.tensor((2 ** i) * np.pi, dtype=torch.float32)
        arg = (c * half[..., r % 3]).double()
        g, = torch.autograd.grad(enc[..., e].sum(), p, retain_graph=True)
        want = torch.zeros_like(g)
        want[..., r % 3] = (torch.cos(arg) if r < 3 else -torch.sin(arg)) * c.double() / 2
        assert torch.equal(enc[..., e].detach(), torch.sin(arg) if r < 3 else torch.cos(arg))
        assert torch.allclose(g, want, rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------- C ABI
def _weights(sdfr):
    """sdfr_fc_weights with every pointer non-null (never dereferenced on the host)."""
    w = sdfr._lib.FcWeights()
    for name, typ in w._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, FAKE)
        elif typ is not ctypes.c_uint32:
            setattr(w, name, typ(*([FAKE] * 7)))
    w.depth, w.width = 8, 256
    return w


def _qargs(sdfr, B=1, R=3, N=32):
    lib = sdfr._lib.lib()
    return sdfr._lib.FcQueryArgs(
        B=B, R=R, N=N, points=FAKE, dirs=FAKE, styles=FAKE, sdf=FAKE, rgb=None, workspace=FAKE,
        workspace_bytes=lib.sdfr_query_fc_workspace_bytes(B, R, N), prepacked=None)


def _gargs(sdfr, B=1, M=40):
    lib = sdfr._lib.lib()
    return sdfr._lib.FcGradArgs(
        B=B, M=M, points=FAKE, styles=FAKE, sdf=None, grad=FAKE, workspace=FAKE,
        workspace_bytes=lib.sdfr_query_fc_grad_workspace_bytes(B, M), prepacked=None)


def _rejected(sdfr, fn, w, a, msg, code=None):
    lib = sdfr._lib.lib()
    rc = getattr(lib, fn)(None if w is None else ctypes.byref(w),
                          None if a is None else ctypes.byref(a), None)
    assert rc == (sdfr._lib.SDFR_EINVAL if code is None else code), (fn, msg, rc)
    err = lib.sdfr_last_error()
    prefix = b"query_fc_grad: " if fn.endswith("grad") else b"query_fc: "
    assert err.startswith(prefix) and msg in err, err


def _weight_rejections(sdfr, fn, args):
    w = _weights(sdfr)
    _rejected(sdfr, fn, None, args(sdfr), b"null args")
    _rejected(sdfr, fn, w, None, b"null args")
    for name in ("pts_w", "pts_b"):
        w2 = _weights(sdfr)
        setattr(w2, name, (ctypes.c_void_p * 7)(*([FAKE] * 5 + [None] + [FAKE])))
        _rejected(sdfr, fn, w2, args(sdfr), b"weight pointer is null")
    for name in ("x_in_w", "x_in_b", "style_w", "style_b", "views_w", "views_b", "sigma_w",
                 "sigma_b", "rgb_w", "rgb_b"):
        w2 = _weights(sdfr)
        setattr(w2, name, None)
        _rejected(sdfr, fn, w2, args(sdfr), b"weight pointer is null")
    w2 = _weights(sdfr)
    w2.sigmoid_beta = None                                  # not read: the next check answers
    a = args(sdfr)
    a.workspace_bytes = 0
    _rejected(sdfr, fn, w2, a, b"workspace too small")
    for field, value in (("depth", 7), ("width", 128)):
        w2 = _weights(sdfr)
        setattr(w2, field, value)
        _rejected(sdfr, fn, w2, args(sdfr), b"needs depth 8, width 256",
                  sdfr._lib.SDFR_EUNSUPPORTED)


def test_library_exports_the_fc_point_calls(sdfr):
    lib = sdfr._lib.lib()
    for name in ("sdfr_query_fc_workspace_bytes", "sdfr_query_fc_forward",
                 "sdfr_query_fc_grad_workspace_bytes", "sdfr_query_fc_grad"):
        assert name in sdfr._lib.EXPORTS and hasattr(lib, name), name
    assert lib.sdfr_abi_version() == 15                      # additive: no version step


def test_fc_query_rejects_bad_arguments_before_any_launch(sdfr):
    fn, w = "sdfr_query_fc_forward", _weights(sdfr)
    _weight_rejections(sdfr, fn, _qargs)
    for zero in ("B", "R", "N"):
        a = _qargs(sdfr)
        setattr(a, zero, 0)
        _rejected(sdfr, fn, w, a, b"empty batch / group / point count")
    for field in ("points", "dirs", "styles", "sdf", "workspace"):
        a = _qargs(sdfr)
        setattr(a, field, None)
        _rejected(sdfr, fn, w, a, b"required pointer is null")
    a = _qargs(sdfr)
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
    # products that wrap in 32 or 64 bits
    for B, R, N in (((1 << 32) - 1,) * 3, (1 << 31, 1, 1 << 26), (1, 1 << 31, 2),
                    (1 << 16, 1 << 16, 1 << 31), (1, (1 << 32) - 1, 1), (1 << 30, 16, 4)):
        a = _qargs(sdfr, B=B, R=R, N=N)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, fn, w, a, b"too many samples per call")


def test_fc_gradient_rejects_bad_arguments_before_any_launch(sdfr):
    fn, w = "sdfr_query_fc_grad", _weights(sdfr)
    _weight_rejections(sdfr, fn, _gargs)
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
    # 2^30 padded points (M rounded up to 8 per face) are the first rejected size
    a = _gargs(sdfr, B=1, M=LIMIT - 7)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, fn, w, a, b"too many points per call")
    a = _gargs(sdfr, B=1, M=LIMIT - 8)
    a.workspace_bytes = 0
    _rejected(sdfr, fn, w, a, b"workspace too small")
    for B, M in (((1 << 32) - 1, (1 << 32) - 1), (1 << 26, 1 << 31), (1, (1 << 32) - 1),
                 (1 << 31, 2)):
        a = _gargs(sdfr, B=B, M=M)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, fn, w, a, b"too many points per call")


def test_fc_workspace_size_functions(sdfr):
    """Both workspaces are the FC render's without segment partials: per-face FiLM slots and
    the render's weight-packing region.  They do not grow with the points, a second face
    adds only its FiLM slots, and they are 0 for zero sizes and at or beyond the limit."""
    lib = sdfr._lib.lib()
    q, g = lib.sdfr_query_fc_workspace_bytes, lib.sdfr_query_fc_grad_workspace_bytes
    pack = lib.sdfr_render_pack_bytes(2)
    # one slice of 16 KiB per k-step of 16 K (4 + 7 x 16 + 18) + row scales and scaled
    # biases of 9 layers
    assert pack == 134 * 16384 + 2 * 9 * 256 * 4
    assert q(0, 3, 32) == q(1, 0, 32) == q(1, 3, 0) == 0
    assert g(0, 40) == g(1, 0) == 0
    assert q(1, 3, 32) == g(1, 40) >= FILM + pack
    assert q(1, 3, 32) < FILM + pack + 512                  # (regions rounded up to 256 B)
    assert q(2, 3, 32) == q(1, 3, 32) + FILM and g(2, 40) == g(1, 40) + FILM
    assert q(5, 3, 32) == q(1, 3, 32) + 4 * FILM and g(5, 40) == g(1, 40) + 4 * FILM
    # no growth with the points
    assert q(1, 1, 1) == q(1, 17, 32) == q(1, 4000, 33)
    assert g(1, 1) == g(1, 9) == g(1, 1 << 20)
    # the point limit: positive one padding unit below, 0 at and beyond it
    assert q(1, (1 << 26) - 16, 16) == q(1, 1, 1) > 0
    assert q(1, (1 << 26) - 15, 16) == 0 == q(1, 1 << 26, 16) == q(1, 16, 1 << 26)
    assert q(1 << 26, 16, 1) == 0 and q((1 << 26) - 1, 16, 1) > 0
    assert q((1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1) == 0 == q(1 << 31, 1, 1 << 26)
    assert g(1, LIMIT - 8) == g(1, 1) > 0
    assert g(1, LIMIT - 7) == 0 == g(1, LIMIT) == g(1 << 26, 1 << 31)
    assert g((1 << 32) - 1, (1 << 32) - 1) == 0 == g(1 << 27, 8) and g((1 << 27) - 1, 8) > 0


def test_query_on_a_cpu_fc_renderer_is_the_module_path(alive):
    """Unchanged behaviour: on CPU tensors an FC renderer's query / query_gradient are the
    network evaluated op by op, exactly; encode_only is the ngp gather's and raises."""
    ren, pts, lat, _ = alive
    assert ren._net_kind() == 2
    pts = pts[:, :5].contiguous()
    B, M = pts.shape[:2]
    dirs = F.normalize(torch.randn(B, M, 3, generator=torch.Generator().manual_seed(6)), dim=-1)
    assert not ren._query_fused_ok(pts, lat)
    with torch.no_grad():
        raw = ren.network(torch.cat([pts, dirs], -1), styles=lat)
        sdf, rgb = ren.query(pts, lat, viewdirs=dirs)
    assert torch.equal(sdf, raw[..., 3]) and torch.equal(rgb, torch.sigmoid(raw[..., :3]))
    want_sdf, want = module_grad(ren, pts, lat)
    with torch.no_grad():
        gs, grad = ren.query_gradient(pts, lat)
    assert np.array_equal(grad.numpy(), want) and np.array_equal(gs.numpy(), want_sdf)
    with pytest.raises(ValueError, match="encode_only"):
        ren.query_gradient(pts, lat, encode_only=True)

"""CPU: the geometry render's C-ABI argument checks and workspace size
(sdfr_render_ngp_geometry, include/sdfr.h) and VolumeFeatureRenderer.render_geometry /
Generator.render_geometry on the op-by-op path: against the reference's SIREN eikonal
fixture, against forward(return_eikonal=True) (also over every sampling flag on a small
SIREN renderer), and on a stub network with a linear SDF."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.golden import weights as W

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch
POINT_LIMIT = 1 << 25  # padded points one call cannot take (the gradient kernels' indexing)


def _weights(sdfr):
    """sdfr_ngp_weights with every pointer non-null (never dereferenced on the host)."""
    w = sdfr._lib.NgpWeights()
    for name, typ in w._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, FAKE)
        elif typ not in (ctypes.c_uint32, ctypes.c_float):
            setattr(w, name, typ(*([FAKE] * 3)))
    w.num_levels, w.base_resolution, w.bound = 16, 16, 2.0
    return w


POINTERS = ("cam", "focal", "near_", "far_", "styles", "pix_x", "pix_y", "t_vals", "workspace")
OUTPUTS = ("sdf", "eikonal", "normal", "depth", "xyz", "mask")


def _args(sdfr, B=1, H=4, W=4, N=3):
    lib = sdfr._lib.lib()
    a = sdfr._lib.NgpGeometryArgs(B=B, H=H, W=W, N=N, t_rand=None, prepacked=None)
    for k in POINTERS + OUTPUTS:
        setattr(a, k, FAKE)
    a.workspace_bytes = lib.sdfr_render_ngp_geometry_workspace_bytes(B, H, W, N)
    return a


def _rejected(sdfr, w, a, msg, code=None):
    lib = sdfr._lib.lib()
    rc = lib.sdfr_render_ngp_geometry(None if w is None else ctypes.byref(w),
                                      None if a is None else ctypes.byref(a), None)
    assert rc == (sdfr._lib.SDFR_EINVAL if code is None else code)
    assert msg in lib.sdfr_last_error(), lib.sdfr_last_error()


def test_geometry_rejects_bad_arguments_before_any_launch(sdfr):
    """1. Every rejection of the header, on fake pointers: nothing is launched."""
    w = _weights(sdfr)
    assert _args(sdfr).workspace_bytes > 0
    _rejected(sdfr, None, _args(sdfr), b"null args")
    _rejected(sdfr, w, None, b"null args")
    for zero in ("B", "H", "W", "N"):
        a = _args(sdfr)
        setattr(a, zero, 0)
        _rejected(sdfr, w, a, b"empty batch / image / sample count")
    for field in POINTERS:
        a = _args(sdfr)
        setattr(a, field, None)
        _rejected(sdfr, w, a, b"required pointer is null")
    a = _args(sdfr)
    for k in OUTPUTS:
        setattr(a, k, None)
    _rejected(sdfr, w, a, b"every output is null")
    for keep in OUTPUTS:                      # any single output passes that check
        a = _args(sdfr)
        for k in OUTPUTS:
            setattr(a, k, FAKE if k == keep else None)
        a.workspace_bytes = 0
        _rejected(sdfr, w, a, b"workspace too small")
    w2 = _weights(sdfr)
    w2.sigma_w = None
    _rejected(sdfr, w2, _args(sdfr), b"weight pointer is null")
    w2 = _weights(sdfr)
    w2.pts_bw = (ctypes.c_void_p * 3)(FAKE, FAKE, None)
    _rejected(sdfr, w2, _args(sdfr), b"FiLM weight pointer is null")
    w2 = _weights(sdfr)
    w2.sigmoid_beta = None                    # a renderer without an SDF
    _rejected(sdfr, w2, _args(sdfr), b"sigmoid_beta is required")
    w2 = _weights(sdfr)
    w2.num_levels = 8
    _rejected(sdfr, w2, _args(sdfr), b"needs 16 levels", sdfr._lib.SDFR_EUNSUPPORTED)
    a = _args(sdfr)
    a.workspace_bytes -= 1
    _rejected(sdfr, w, a, b"workspace too small")
    # B x (H W N rounded up to 8) >= 2^25 is the first rejected size; one padding unit
    # below passes that check and reaches the workspace check
    for B, H, W_, N in ((1, 1, 1, POINT_LIMIT - 7), (1, 1 << 10, 1 << 10, 32), (4, 512, 512, 32),
                        (3, 1, 1, (POINT_LIMIT // 3 + 8) // 8 * 8),
                        # products that wrap in 32 or 64 bits
                        (1, 1 << 16, 1 << 16, 1), (1, 1 << 16, 1 << 16, 1 << 16),
                        ((1 << 32) - 1,) * 4, (1 << 31, 1, 1, 1 << 26), (1, 1 << 31, 2, 1),
                        (1, 3, (1 << 32) - 1, (1 << 32) - 1)):
        a = _args(sdfr, B, H, W_, N)
        assert a.workspace_bytes == 0, (B, H, W_, N)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, w, a, b"too many points per call")
    a = _args(sdfr, 1, 1, 1, POINT_LIMIT - 8)
    assert a.workspace_bytes > 0
    a.workspace_bytes = 0
    _rejected(sdfr, w, a, b"workspace too small")


def test_geometry_workspace_is_the_gradient_workspace_plus_sample_regions(sdfr):
    """2. The gradient call's workspace for (B, H W N) plus 36 bytes per padded point in
    four regions (points 12, (z, dist) 8, sdf 4, gradient 12), each rounded up to 256."""
    lib = sdfr._lib.lib()
    ws = lib.sdfr_render_ngp_geometry_workspace_bytes
    grad = lib.sdfr_query_ngp_grad_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731

    def regions(B, M):
        P = B * ((M + 7) // 8 * 8)
        return sum(up(P * k) for k in (12, 8, 4, 12))

    for B, H, W_, N in ((1, 1, 1, 1), (1, 5, 5, 3), (2, 8, 8, 24), (3, 8, 8, 24), (32, 64, 64, 24),
                        (1, 128, 128, 128), (1, 3, 8, 24), (1, 1, 1, POINT_LIMIT - 8)):
        assert ws(B, H, W_, N) == grad(B, H * W_ * N) + regions(B, H * W_ * N), (B, H, W_, N)
    # 512 + 36 bytes per padded point where no region needs rounding (64 points a step)
    assert ws(1, 8, 8, 2) - ws(1, 8, 8, 1) == 64 * (512 + 36)
    assert ws(1, 16, 8, 24) - ws(1, 8, 8, 24) == 8 * 8 * 24 * (512 + 36)
    assert ws(1, 1, 1, 1) == ws(1, 1, 1, 8) == ws(1, 2, 2, 2)       # one padding unit
    assert ws(1, 1, 3, 3) > ws(1, 1, 1, 8)
    # the first rejected size has no workspace size; one padding unit below has
    assert ws(1, 1, 1, POINT_LIMIT - 7) == 0 == ws(1, 1 << 10, 1 << 10, 32)
    assert ws(1, 1, 1, POINT_LIMIT - 8) > 512 * (POINT_LIMIT - 8)
    assert ws(0, 4, 4, 4) == 0 == ws(1, 4, 4, 0)
    assert ws((1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1) == 0


# --------------------------------------------------------------------------------------
def _stage1_generator_cpu(sdfr, golden_dir, g, kind):
    """tests/test_gpu_stage1.py's _stage1_generator on the CPU."""
    opt = sdfr.vol_render_opt(ngp=kind == "ngp", train_renderer=True)
    opt.model.renderer_spatial_output_dim = int(g["res"])
    opt.rendering.N_samples = int(g["n_samples"])
    gen = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False)
    own = gen.state_dict()
    sd = W.det_state_dict(W.golden_entries(golden_dir, kind=kind), "")
    sd = {k: v for k, v in sd.items() if k in own}
    assert set(sd) == set(own)
    gen.load_state_dict(sd, strict=True)
    return gen


def _rel_err(got, ref):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    ref = np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def test_render_geometry_module_path_vs_reference_siren(sdfr, golden_dir):
    """3. The SIREN stage-1 generator of eikonal_siren.npz on the CPU: Generator.
    render_geometry's eikonal / sdf against the reference's own (the project's relative
    bounds for these tensors, tests/test_gpu_stage1.py), the eikonal term exactly
    forward(return_eikonal=True)'s, xyz and mask exactly forward's."""
    g = np.load(golden_dir / "eikonal_siren.npz")
    gen = _stage1_generator_cpu(sdfr, golden_dir, g, "siren")
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    tr = t("t_rand")
    geo = gen.render_geometry([t("z")], t("ext"), t("focal"), t("near"), t("far"), t_rand=tr,
                              want=("sdf", "eikonal", "xyz", "mask"))
    assert isinstance(geo, sdfr.Geometry)
    assert geo.normal is None and geo.depth is None
    assert geo.sdf.shape == g["sdf"].shape and geo.eikonal.shape == g["eikonal"].shape
    assert geo.xyz.shape == (2, 3, 8, 8) and geo.mask.shape == (2, 1, 8, 8)
    for v in (geo.sdf, geo.eikonal, geo.xyz, geo.mask):
        assert not v.requires_grad and v.grad_fn is None
    e_eik, e_sdf = _rel_err(geo.eikonal, g["eikonal"]), _rel_err(geo.sdf, g["sdf"])
    print(f"module path vs reference: eikonal {e_eik:.3e} sdf {e_sdf:.3e} (relative)")
    assert e_eik <= 1e-4 and e_sdf <= 2e-5
    ren = gen.renderer
    ren.return_xyz, ren.return_sdf = True, True
    lat = gen.styles_and_noise_forward([t("z")])[0]
    _, _, sdf, mask, xyz, eik = ren(t("ext"), t("focal"), t("near"), t("far"), styles=lat,
                                    return_eikonal=True, t_rand=tr)
    assert eik.requires_grad                       # forward keeps its autograd dispatch
    assert torch.equal(geo.eikonal, eik.detach())
    assert torch.equal(geo.sdf, sdf.detach())
    assert torch.equal(geo.xyz, xyz.detach()) and torch.equal(geo.mask, mask.detach())


class _LinearSdf(torch.nn.Module):
    """raw[..., 3] = a . p_net + c; everything else zero."""

    def __init__(self, a, c):
        super().__init__()
        self.register_buffer("a", torch.tensor(a, dtype=torch.float32))
        self.c = c

    def forward(self, x, styles):
        sdf = x[..., :3] @ self.a + self.c
        out = torch.zeros(x.shape[:-1] + (4,), dtype=x.dtype)
        return torch.cat([out[..., :3], sdf.unsqueeze(-1)], -1)


A, C = (0.3, -0.2, 0.5), 0.05


def _stub_renderer(sdfr, res, N, **flags):
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    r = opt.rendering
    r.N_samples = N
    r.perturb = 0
    for k, v in flags.items():
        r[k] = v
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res).eval()
    if not flags.get("no_sdf"):
        ren.network = _LinearSdf(A, C)
    return ren


def _weights64(ren, sdf, z, rays_d, force_background):
    """The reference's weight formula (sdf_model.py:236-301) in float64."""
    sdf, z = sdf.double()[..., 0], z.double()
    dn = rays_d.double().norm(dim=-1, keepdim=True)
    dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)], -1) * dn
    beta = float(ren.sigmoid_beta.detach())
    sigma = torch.sigmoid(-sdf / beta) / beta
    alpha = 1 - torch.exp(-sigma * dists)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1 - alpha + 1e-10], -1),
                      -1)[..., :-1]
    w = alpha * T
    if force_background:
        w[..., -1] = 1 - w[..., :-1].sum(-1)
    return w


@pytest.mark.parametrize("force_background", [False, True])
def test_render_geometry_on_a_linear_sdf(sdfr, force_background):
    """4. sdf = a . p_net + c: eikonal = a 2 / (far - near) everywhere, normal = eikonal
    sum(w), depth = the test's own float64 sum(w z); force_background makes sum(w) = 1."""
    res, N, B = 5, 6, 2
    ren = _stub_renderer(sdfr, res, N, force_background=force_background)
    torch.manual_seed(1)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.zeros(B, 256)
    with torch.no_grad():
        geo = ren.render_geometry(ext, focal, near, far, lat,
                                  want=("normal", "depth", "xyz", "mask", "sdf", "eikonal"))
        unit = ren.render_geometry(ext, focal, near, far, lat, want=("normal",), normalize=True)
    for v in geo:
        assert not v.requires_grad and v.grad_fn is None
    for v in (ext, focal, near, far, lat):
        assert not v.requires_grad and v.grad is None
    assert geo.sdf.shape == (B, res, res, N, 1) and geo.eikonal.shape == (B, res, res, N, 3)
    span = (far - near).reshape(B, 1, 1, 1, 1)
    want_eik = (torch.tensor(A) * 2 / span).expand(B, res, res, N, 3)
    # the chain rule's two roundings (x 2, / span) in either order
    torch.testing.assert_close(geo.eikonal, want_eik, rtol=3 * 2.0 ** -24, atol=0)
    # the weights in float64 from the call's own SDF and the renderer's rays and depths
    _, rays_d, _ = ren.get_rays(focal, ext)
    nr, fr = near.reshape(B, 1, 1, 1), far.reshape(B, 1, 1, 1)
    z = (nr * (1. - ren.t_vals) + fr * ren.t_vals).expand(B, res, res, N)
    w = _weights64(ren, geo.sdf, z, rays_d, force_background)
    wsum = w.sum(-1)
    if force_background:
        torch.testing.assert_close(wsum, torch.ones_like(wsum), rtol=0, atol=1e-12)
    else:
        # the 1e10 last segment absorbs what is left; a real transition in front of it
        front = w[..., :-1].sum(-1)
        print(f"front weight sum {float(front.min()):.3f} .. {float(front.max()):.3f}")
        assert 0.01 < float(front.min()) < 0.3 and 0.5 < float(front.max()) < 0.999
    # fp32 rounding of a front-to-back composite of N terms: the s-th weight carries
    # about s + 4 roundings (exp, sigmoid, divisions, the running product) and the sum
    # N more: (2 N + 4) eps of the largest map value, eps = 2^-24
    eps_n = (2 * N + 4) * 2.0 ** -24
    depth64 = (w * z.double()).sum(-1)
    d_err = float((geo.depth[:, 0].double() - depth64).abs().max())
    print(f"depth err {d_err:.3e} (bound {eps_n * float(depth64.max()):.3e})")
    assert d_err <= eps_n * float(depth64.max())
    normal64 = want_eik[..., 0, :].double() * wsum.unsqueeze(-1)
    n_err = float((geo.normal.permute(0, 2, 3, 1).double() - normal64).abs().max())
    assert n_err <= eps_n * float(normal64.abs().max())
    torch.testing.assert_close(geo.mask[:, 0].double(), w[..., -1], rtol=0, atol=eps_n)
    pts64 = ext[:, None, None, None, :3, 3].double() + rays_d.double().unsqueeze(3) * \
        z.double().unsqueeze(-1)
    xyz64 = (w.unsqueeze(-1) * pts64).sum(3)
    x_err = float((geo.xyz.permute(0, 2, 3, 1).double() - xyz64).abs().max())
    assert x_err <= eps_n * float(xyz64.abs().max()) + 2.0 ** -24 * float(pts64.abs().max())
    # normalize=True: unit vectors along a
    n = unit.normal
    assert unit.depth is None and unit.sdf is None
    torch.testing.assert_close(n.norm(dim=1), torch.ones(B, res, res), rtol=0, atol=1e-6)
    a_unit = torch.tensor(A) / torch.tensor(A).norm()
    torch.testing.assert_close(n.permute(0, 2, 3, 1), a_unit.expand(B, res, res, 3), rtol=0,
                               atol=1e-6)
    assert torch.equal(n, geo.normal / geo.normal.norm(dim=1, keepdim=True).clamp_min(1e-20))


def test_render_geometry_grad_mode_and_argument_errors(sdfr):
    """4b. With grad enabled and inputs that require grad the result still carries no graph
    and the caller's tensors get no .grad; no_sdf and unknown fields raise."""
    res, N, B = 4, 3, 1
    ren = _stub_renderer(sdfr, res, N)
    torch.manual_seed(2)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.zeros(B, 256, requires_grad=True)
    ext = ext.clone().requires_grad_(True)
    geo = ren.render_geometry(ext, focal, near, far, lat, want=("normal", "eikonal"))
    assert geo.depth is None and geo.xyz is None and geo.mask is None and geo.sdf is None
    assert not geo.normal.requires_grad and not geo.eikonal.requires_grad
    assert ext.requires_grad and ext.grad is None and lat.grad is None
    with torch.no_grad():
        same = ren.render_geometry(ext, focal, near, far, lat, want=("normal", "eikonal"))
    assert torch.equal(same.normal, geo.normal) and torch.equal(same.eikonal, geo.eikonal)
    with pytest.raises(ValueError, match="want"):
        ren.render_geometry(ext, focal, near, far, lat, want=("colour",))
    with pytest.raises(ValueError, match="want"):
        ren.render_geometry(ext, focal, near, far, lat, want=())
    plain = _stub_renderer(sdfr, res, N, no_sdf=True)
    with pytest.raises(ValueError, match="no_sdf"):
        plain.render_geometry(ext, focal, near, far, lat)


def test_render_geometry_shares_forward_samples_and_weights(sdfr):
    """5. A small SIREN renderer over perturb x no_offset_sampling x force_background x
    no_z_normalize, t_rand given: render_geometry's sdf, eikonal, xyz and mask are
    forward(return_eikonal=True)'s bit for bit -- the two paths place their samples and
    form their weights in the same code."""
    B, res, N, style_dim = 2, 4, 3, 32
    for perturb, no_offset, background, no_z in itertools.product((0, 1), repeat=4):
        flags = dict(perturb=perturb, no_offset_sampling=bool(no_offset),
                     force_background=bool(background), no_z_normalize=bool(no_z))
        r = sdfr.vol_render_opt(ngp=False).rendering
        r.depth, r.width, r.N_samples = 2, 32, N
        r.return_sdf, r.return_xyz = True, True
        for k, v in flags.items():
            r[k] = v
        torch.manual_seed(3)
        ren = sdfr.VolumeFeatureRenderer(r, style_dim=style_dim, out_im_res=res, mode="train")
        assert isinstance(ren.network, sdfr.renderer.SirenGenerator) and ren.perturb == perturb
        ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
        lat = torch.randn(B, style_dim)
        tr = torch.rand((B, res, res, N) if no_offset else (B, res, res))
        _, _, sdf, mask, xyz, eik = ren(ext, focal, near, far, styles=lat, return_eikonal=True,
                                        t_rand=tr)
        geo = ren.render_geometry(ext, focal, near, far, lat, t_rand=tr,
                                  want=("sdf", "eikonal", "xyz", "mask"))
        assert float(geo.eikonal.abs().max()) > 0 and float(geo.mask.abs().max()) > 0, flags
        assert torch.equal(geo.sdf, sdf.detach()), flags
        assert torch.equal(geo.eikonal, eik.detach()), flags
        assert torch.equal(geo.xyz, xyz.detach()), flags
        assert torch.equal(geo.mask, mask.detach()), flags

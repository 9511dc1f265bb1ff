"""CPU: the surface render's C-ABI argument checks and workspace sizes
(sdfr_render_ngp_surface, sdfr_render_siren_surface, include/sdfr.h) and
VolumeFeatureRenderer.render_surface / Generator.render_surface / shade_surface on the
op-by-op path: a plane SDF on a stub network against the analytic crossing, the SIREN
network against the bracket of the reference's own per-sample SDF, and the miss cases."""
import ctypes

import numpy as np
import pytest
import torch

from tests.golden import weights as W

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch
LIMITS = {"ngp": 1 << 25, "siren": 1 << 30}     # padded points one call cannot take
EPS = 2.0 ** -23

POINTERS = ("cam", "focal", "near_", "far_", "styles", "pix_x", "pix_y", "t_vals", "workspace")
OUTPUTS = ("hit", "sample", "depth", "residual", "xyz", "normal", "rgb", "sdf")
NETS = ("ngp", "siren")


def _weights(sdfr, net):
    """The network's weight struct with every pointer non-null (never dereferenced)."""
    w = (sdfr._lib.NgpWeights if net == "ngp" else sdfr._lib.SirenWeights)()
    for name, typ in w._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, FAKE)
        elif typ not in (ctypes.c_uint32, ctypes.c_float):
            setattr(w, name, typ(*([FAKE] * (3 if net == "ngp" else 8))))
    if net == "ngp":
        w.num_levels, w.base_resolution, w.bound = 16, 16, 2.0
    else:
        w.depth, w.width = 8, 256
    return w


def _size(sdfr, net):
    return getattr(sdfr._lib.lib(), f"sdfr_render_{net}_surface_workspace_bytes")


def _args(sdfr, net, B=1, H=4, W=4, N=3):
    a = sdfr._lib.SurfaceArgs(B=B, H=H, W=W, N=N, t_rand=None, refine_steps=8, prepacked=None,
                              prepacked_grad=None)
    for k in POINTERS + OUTPUTS:
        setattr(a, k, FAKE)
    a.workspace_bytes = _size(sdfr, net)(B, H, W, N)
    return a


def _rejected(sdfr, net, w, a, msg, code=None):
    lib = sdfr._lib.lib()
    rc = getattr(lib, f"sdfr_render_{net}_surface")(None if w is None else ctypes.byref(w),
                                                    None if a is None else ctypes.byref(a), None)
    assert rc == (sdfr._lib.SDFR_EINVAL if code is None else code), (net, msg, rc)
    err = lib.sdfr_last_error()
    assert err.startswith(f"render_{net}_surface: ".encode()) and msg in err, err


@pytest.mark.parametrize("net", NETS)
def test_surface_rejects_bad_arguments_before_any_launch(sdfr, net):
    """1. Every rejection of the header, on fake pointers: nothing is launched."""
    w = _weights(sdfr, net)
    assert _args(sdfr, net).workspace_bytes > 0
    _rejected(sdfr, net, None, _args(sdfr, net), b"null args")
    _rejected(sdfr, net, w, None, b"null args")
    for zero in ("B", "H", "W", "N"):
        a = _args(sdfr, net)
        setattr(a, zero, 0)
        _rejected(sdfr, net, w, a, b"empty batch / image / sample count")
    for field in POINTERS:
        a = _args(sdfr, net)
        setattr(a, field, None)
        _rejected(sdfr, net, w, a, b"required pointer is null")
    a = _args(sdfr, net)
    for k in OUTPUTS:
        setattr(a, k, None)
    _rejected(sdfr, net, w, a, b"every output is null")
    for keep in OUTPUTS:                      # any single output passes that check
        a = _args(sdfr, net)
        for k in OUTPUTS:
            setattr(a, k, FAKE if k == keep else None)
        a.workspace_bytes = 0
        _rejected(sdfr, net, w, a, b"workspace too small")
    for steps in (33, (1 << 32) - 1):
        a = _args(sdfr, net)
        a.refine_steps = steps
        _rejected(sdfr, net, w, a, b"refine_steps must be 0..32")
    for steps in (0, 32):                     # both ends of the range pass that check
        a = _args(sdfr, net)
        a.refine_steps = steps
        a.workspace_bytes -= 1
        _rejected(sdfr, net, w, a, b"workspace too small")
    w2 = _weights(sdfr, net)
    w2.sigma_w = None
    _rejected(sdfr, net, w2, _args(sdfr, net), b"weight pointer is null")
    w2 = _weights(sdfr, net)
    n = 3 if net == "ngp" else 8
    w2.pts_bw = (ctypes.c_void_p * n)(*([FAKE] * (n - 1) + [None]))
    _rejected(sdfr, net, w2, _args(sdfr, net), b"FiLM weight pointer is null")
    w2 = _weights(sdfr, net)
    if net == "ngp":
        w2.num_levels = 8
        _rejected(sdfr, net, w2, _args(sdfr, net), b"needs 16 levels", sdfr._lib.SDFR_EUNSUPPORTED)
    else:
        w2.depth = 4
        _rejected(sdfr, net, w2, _args(sdfr, net), b"needs depth 8", sdfr._lib.SDFR_EUNSUPPORTED)
        w2 = _weights(sdfr, net)
        w2.width = 128
        _rejected(sdfr, net, w2, _args(sdfr, net), b"needs depth 8", sdfr._lib.SDFR_EUNSUPPORTED)
    w2 = _weights(sdfr, net)
    w2.sigmoid_beta = None                    # not read, not required
    a = _args(sdfr, net)
    a.workspace_bytes -= 1
    _rejected(sdfr, net, w2, a, b"workspace too small")
    # H W N at the limit is the first rejected size, also through products that wrap
    lim = LIMITS[net]
    for B, H, W_, N in ((1, 1, 1, lim), (1, 1 << 10, 1 << 10, lim >> 20), (4, 1 << 9, 1 << 9, lim >> 20),
                        (1, 1 << 16, 1 << 16, 1), (1, 1 << 16, 1 << 16, 1 << 16),
                        ((1 << 32) - 1,) * 4, (1 << 31, 1, 1, 1 << 26), (1, 1 << 31, 2, 1),
                        (1, 3, (1 << 32) - 1, (1 << 32) - 1)):
        a = _args(sdfr, net, B, H, W_, N)
        assert a.workspace_bytes == 0, (B, H, W_, N)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, net, w, a, b"too many points per call")


def _up(v, m=256):
    return (v + m - 1) // m * m


def surface_layout(lib, net, B, H, W_, N):
    """The workspace layout the header documents: the offset of every region by name, and
    "total".  M = H W, Mp = M up to 32, S = B M N, rays = B M, P = B Mp."""
    M = H * W_
    Mp = _up(M, 32)
    if net == "ngp":
        Pq = max(_up(M, 16) * N, _up(Mp // 32, 16) * 32)
        head = [("evaluations", lib.sdfr_query_ngp_workspace_bytes(B, 16, Pq // 16)),
                ("gradient", lib.sdfr_query_ngp_grad_workspace_bytes(B, M))]
    else:
        head = [("evaluations", lib.sdfr_query_siren_workspace_bytes(B, M, N)),
                ("gradient", lib.sdfr_query_siren_grad_workspace_bytes(B, M))]
    S, rays, P = B * M * N, B * M, B * Mp
    regions = head + [("points", 12 * S), ("z_dist", 8 * S), ("sdf", 4 * S),
                      ("brackets", 16 * rays), ("sample", 4 * rays), ("z_star", 4 * rays),
                      ("midpoints", 12 * P), ("midpoint_sdf", 4 * P), ("hit_points", 12 * rays),
                      ("directions", 12 * rays), ("grad_sdf", 4 * rays), ("grad", 12 * rays),
                      ("colour_sdf", 4 * rays), ("colour", 12 * rays)]
    out, off = {}, 0
    for name, nbytes in regions:
        out[name] = off
        off += _up(nbytes)
    out["total"] = off
    return out


@pytest.mark.parametrize("net", NETS)
def test_surface_workspace_follows_the_documented_layout(sdfr, net):
    """2. The header's formula: the evaluations' region, the gradient's region, then the
    per-sample, per-ray and per-midpoint regions, each rounded up to 256 bytes; 0 at and
    beyond the point limits."""
    lib = sdfr._lib.lib()
    ws, lim = _size(sdfr, net), LIMITS[net]

    def formula(B, H, W_, N):
        return surface_layout(lib, net, B, H, W_, N)["total"]

    for shape in ((1, 1, 1, 1), (1, 5, 5, 3), (2, 3, 3, 1), (2, 8, 8, 24), (1, 3, 3, 130),
                  (32, 64, 64, 24), (1, 128, 128, 128), (1, 3, 8, 24), (1, 1, 1, lim // 16 - 1),
                  (1, 4, 4, lim // 16 - 1)):
        assert ws(*shape) == formula(*shape) > 0, shape
    # one ray is a tile of 16 padded groups: 16 N is the count that meets the limit
    assert ws(1, 1, 1, lim // 16) == 0 == ws(1, 4, 4, lim // 16) == ws(1, 1, 1, lim)
    assert ws(1, 1 << 10, 1 << 10, lim >> 20) == 0
    assert ws(2, 1 << 10, 1 << 10, lim >> 21) == 0                 # B x the padded count
    assert ws(1, 1 << 10, 1 << 10, (lim >> 20) - 1) > 0
    assert ws(0, 4, 4, 4) == 0 == ws(1, 4, 4, 0) == ws(1, 0, 4, 4)
    assert ws((1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1) == 0


# --------------------------------------------------------------------------------------
class _PlaneSdf(torch.nn.Module):
    """raw[..., 3] = n . p_net + c and a constant colour logit; float64 inside, so the
    plane's own evaluation error is one rounding of the result."""

    def __init__(self, n, c):
        super().__init__()
        self.register_buffer("n", torch.tensor(n, dtype=torch.float64))
        self.c = c

    def forward(self, x, styles):
        sdf = (x[..., :3].double() @ self.n + self.c).to(x.dtype)
        rgb = torch.full(x.shape[:-1] + (3,), 0.5, dtype=x.dtype) + 0 * x[..., 3:6]
        return torch.cat([rgb, sdf.unsqueeze(-1)], -1)


# the plane n . p + c = 0 in world units: about 0.12 in front of the origin as the cameras
# see it, so that it cuts the sampled depth range [0.88, 1.08] for part of a 5 x 5 image
PLANE_N, PLANE_C = (0.3, -0.2, 1.0), -0.12


def _stub_renderer(sdfr, res, N, **flags):
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    r = opt.rendering
    r.N_samples = N
    r.perturb = 0
    for k, v in flags.items():
        r[k] = v
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res).eval()
    if not flags.get("no_sdf"):
        ren.network = _PlaneSdf(PLANE_N, PLANE_C)
    return ren


ALL = ("hit", "sample", "depth", "xyz", "normal", "rgb", "residual", "sdf")


@pytest.mark.parametrize("steps", [0, 8])
@pytest.mark.parametrize("no_z", [False, True])
def test_render_surface_on_a_plane(sdfr, steps, no_z):
    """3. sdf = n . p_net + c along a ray o + d z is linear in z: sdf(z) = A + S z with
    S = n . d_net < 0 (the camera looks into the half space), so the crossing is z0 = -A / S
    for the rays where it lies between the first and the last sample, and a miss elsewhere.
    hit and sample are exact; depth is within the evaluation error of f over the slope plus
    the roundings of the chain; the normal is n / |n|."""
    res, N, B = 5, 6, 2
    # the plane is placed so that part of the image crosses it inside [near, far)
    ren = _stub_renderer(sdfr, res, N, no_z_normalize=no_z)
    torch.manual_seed(1)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.zeros(B, 256)
    scale = 1.0 if no_z else float(2 / (far - near).reshape(-1)[0])
    # c in network units; chosen per mode so that the plane cuts the sampled depth range
    ren.network.c = PLANE_C * scale
    out = ren.render_surface(ext, focal, near, far, lat, refine_steps=steps, want=ALL)
    assert isinstance(out, sdfr.Surface)
    for v in out:
        assert not v.requires_grad and v.grad_fn is None
    assert out.hit.shape == (B, 1, res, res) == out.sample.shape == out.depth.shape
    assert out.xyz.shape == (B, 3, res, res) == out.normal.shape == out.rgb.shape
    assert out.sdf.shape == (B, res, res, N, 1) and out.sample.dtype == torch.int32

    rays_o, rays_d, _ = ren.get_rays(focal, ext)
    span = (far - near).reshape(B, 1, 1, 1).double()
    k = torch.ones_like(span) if no_z else 2 / span
    n = torch.tensor(PLANE_N, dtype=torch.float64)
    A = (rays_o.double() * k) @ n + ren.network.c            # sdf at z = 0
    S = (rays_d.double() * k) @ n                             # d sdf / d z
    z0 = -A / S
    assert (S < 0).all()
    z = (near.reshape(B, 1, 1, 1) * (1. - ren.t_vals) + far.reshape(B, 1, 1, 1) * ren.t_vals)
    z = z.expand(B, res, res, N).double()
    # analytic bracket: the last sample in front of the plane; rays whose crossing is within
    # 1e-6 of a sample are not placed (the fp32 SDF there may fall on either side)
    sdf64 = A.unsqueeze(-1) + S.unsqueeze(-1) * z
    assert float(sdf64.abs().min()) > 1e-6
    cross = (sdf64[..., :-1] > 0) & (sdf64[..., 1:] <= 0)
    want_hit = cross.any(-1)
    want_s = torch.where(want_hit, cross.int().argmax(-1), torch.full_like(cross[..., 0].int(), -1))
    assert 0 < int(want_hit.sum()) < want_hit.numel()        # hits and misses
    assert torch.equal(out.hit[:, 0], want_hit.float())
    assert torch.equal(out.sample[:, 0], want_s.int())
    assert torch.equal(out.sdf[..., 0], ren.render_surface(ext, focal, near, far, lat,
                                                           want=("sdf",)).sdf[..., 0])
    hit = want_hit
    # |depth - z0| <= 8 eps ((|c| + |n| |p_net|) / |n . d_net| + |z0|)
    p_net = (rays_o.double() + rays_d.double() * z0.unsqueeze(-1)) * k
    bound = 8 * EPS * ((abs(ren.network.c) + n.norm() * p_net.norm(dim=-1)) / S.abs() + z0.abs())
    err = (out.depth[:, 0].double() - z0).abs()
    print(f"steps {steps} no_z {no_z}: depth err {float(err[hit].max()):.3e} "
          f"(bound {float(bound[hit].min()):.3e} .. {float(bound[hit].max()):.3e})")
    assert (err[hit] <= bound[hit]).all()
    unit = (n / n.norm()).float()
    nrm = out.normal.permute(0, 2, 3, 1)
    assert float((nrm[hit] - unit).abs().max()) <= 16 * EPS
    want_xyz = rays_o + rays_d * out.depth[:, 0].unsqueeze(-1)
    assert torch.equal(out.xyz.permute(0, 2, 3, 1)[hit], want_xyz[hit])
    assert float(out.residual[:, 0][hit].abs().max()) <= float((bound * S.abs())[hit].max()) + 4 * EPS
    assert torch.equal(out.rgb.permute(0, 2, 3, 1)[hit],
                       torch.sigmoid(torch.full((int(hit.sum()), 3), 0.5)))
    for key in ("depth", "xyz", "normal", "rgb", "residual"):
        v = getattr(out, key).permute(0, 2, 3, 1)
        assert (v[~hit] == 0).all(), key


# --------------------------------------------------------------------------------------
def _siren_cpu(sdfr, golden_dir, res, N, **flags):
    opt = sdfr.vol_render_opt(ngp=False)
    r = opt.rendering
    r.N_samples = N
    for k, v in flags.items():
        r[k] = v
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res)
    sd = W.det_state_dict(W.golden_entries(golden_dir, siren=True), "renderer.")
    own = ren.state_dict()
    ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()
                         if k[len("renderer."):] in own}, strict=True)
    return ren.eval()


def numpy_bracket(sdf):
    """hit [..] and s* [..] (-1: a miss) of sdf [.., N]: the definition's step 1."""
    sdf = np.asarray(sdf)
    if sdf.shape[-1] < 2:
        return np.zeros(sdf.shape[:-1], bool), np.full(sdf.shape[:-1], -1, np.int32)
    cross = (sdf[..., :-1] > 0) & (sdf[..., 1:] <= 0)
    hit = cross.any(-1)
    return hit, np.where(hit, cross.argmax(-1), -1).astype(np.int32)


@pytest.fixture(scope="module")
def siren_case(sdfr, golden_dir):
    g = np.load(golden_dir / "render_siren_mesh_opts.npz")
    ren = _siren_cpu(sdfr, golden_dir, int(g["res"]), int(g["n_samples"]), static_viewdirs=True,
                     force_background=True, perturb=0)
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    return g, ren, (t("ext"), t("focal"), t("near"), t("far"), t("latent"))


def test_module_surface_on_the_siren_vs_reference_sdf(siren_case):
    """4. render_siren_mesh_opts (8 x 8, N = 32) on the CPU: hit and sample equal the
    bracket of the reference's own per-sample SDF, except on rays whose bracketing samples
    have |sdf| < 2e-5 (the project's SDF bound against the reference: the sign there is not
    pinned); at most 5 % of the rays may be set aside.  Every ray of this fixture crosses."""
    g, ren, inputs = siren_case
    with torch.no_grad():
        out = ren.render_surface(*inputs, want=("hit", "sample", "sdf", "depth", "normal"))
    ref = g["sdf"][..., 0]
    hit, s = numpy_bracket(ref)
    assert hit.all()
    at = np.take_along_axis(np.abs(ref), np.stack([s, s + 1], -1).astype(np.int64), -1)
    # a sample of the reference within the bound of zero anywhere before the bracket could
    # move the first crossing too: set those rays aside as well
    before = np.arange(ref.shape[-1]) <= (s + 1)[..., None]
    unsure = (at < 2e-5).any(-1) | ((np.abs(ref) < 2e-5) & before).any(-1)
    print(f"rays set aside: {int(unsure.sum())} of {unsure.size}")
    assert unsure.mean() <= 0.05
    keep = ~unsure
    assert np.array_equal(out.hit[:, 0].numpy()[keep], hit[keep].astype(np.float32))
    assert np.array_equal(out.sample[:, 0].numpy()[keep], s[keep])
    assert float(np.abs(out.sdf.numpy() - g["sdf"]).max()) <= 2e-5
    own_hit, own_s = numpy_bracket(out.sdf[..., 0].numpy())
    assert np.array_equal(out.hit[:, 0].numpy(), own_hit.astype(np.float32))
    assert np.array_equal(out.sample[:, 0].numpy(), own_s)
    torch.testing.assert_close(out.normal.norm(dim=1), torch.ones_like(out.hit[:, 0]),
                               rtol=0, atol=4 * EPS)
    # the depth lies inside its bracket of samples
    rays = ren.camera_rays(inputs[1], inputs[0], inputs[2], inputs[3])
    z = ren.sample_points(rays[0], rays[1], rays[3], rays[4], None, None)[0]
    z = z.expand(out.sdf.shape[:-1])
    lo = z.gather(-1, torch.from_numpy(own_s).long().unsqueeze(-1))[..., 0]
    hi = z.gather(-1, torch.from_numpy(own_s).long().unsqueeze(-1) + 1)[..., 0]
    assert ((out.depth[:, 0] >= lo) & (out.depth[:, 0] <= hi)).all()


def test_module_surface_refinement_shrinks_the_residual(siren_case):
    """K = 8 bisection steps leave a smaller mean |sdf| at the hit than K = 0."""
    _, ren, inputs = siren_case
    with torch.no_grad():
        r0 = ren.render_surface(*inputs, refine_steps=0, want=("hit", "residual"))
        r8 = ren.render_surface(*inputs, refine_steps=8, want=("hit", "residual"))
    assert torch.equal(r0.hit, r8.hit)
    m0, m8 = float(r0.residual.abs().mean()), float(r8.residual.abs().mean())
    print(f"mean |residual|: K=0 {m0:.3e} K=8 {m8:.3e}")
    assert m8 < m0


def test_module_surface_miss_cases(sdfr, golden_dir, siren_case):
    """5a. sigma_linear.bias shifted by +1 / -1 (all outside / all inside) and N_samples = 1:
    every ray is a miss, every float map is zero and sample is -1."""
    g, ren, inputs = siren_case
    maps = ("hit", "sample", "depth", "xyz", "normal", "rgb", "residual")

    def all_miss(r):
        with torch.no_grad():
            out = r.render_surface(*inputs, want=maps)
        assert (out.sample == -1).all()
        for key in maps:
            if key != "sample":
                assert (getattr(out, key) == 0).all(), key

    bias = ren.network.sigma_linear.bias
    for shift in (1.0, -1.0):
        with torch.no_grad():
            bias += shift
        try:
            all_miss(ren)
        finally:
            with torch.no_grad():
                bias -= shift
    one = _siren_cpu(sdfr, golden_dir, int(g["res"]), 1, static_viewdirs=True, perturb=0)
    all_miss(one)


def test_render_surface_argument_errors_and_grad_mode(sdfr):
    """5b. Unknown fields, an empty want, refine_steps outside 0..32 and a renderer without
    an SDF raise; inputs that require grad leave no graph and get no .grad."""
    res, N, B = 4, 3, 1
    ren = _stub_renderer(sdfr, res, N)
    torch.manual_seed(2)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.zeros(B, 256, requires_grad=True)
    ext = ext.clone().requires_grad_(True)
    out = ren.render_surface(ext, focal, near, far, lat, want=("normal", "depth"))
    assert out.hit is None and out.rgb is None and out.sdf is None
    assert not out.normal.requires_grad and not out.depth.requires_grad
    assert ext.grad is None and lat.grad is None
    for bad in (("colour",), ()):
        with pytest.raises(ValueError, match="want"):
            ren.render_surface(ext, focal, near, far, lat, want=bad)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="refine_steps"):
            ren.render_surface(ext, focal, near, far, lat, refine_steps=bad)
    plain = _stub_renderer(sdfr, res, N, no_sdf=True)
    with pytest.raises(ValueError, match="no_sdf"):
        plain.render_surface(ext, focal, near, far, lat)


def test_generator_render_surface_maps_styles_then_renders(sdfr):
    """5c. Generator.render_surface = the mapping network and truncation of forward, then
    renderer.render_surface on the mapped latent."""
    opt = sdfr.vol_render_opt(ngp=False)
    opt.model.renderer_spatial_output_dim = 4
    opt.rendering.N_samples = 6
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).eval()
    res = g.renderer.out_im_res
    z = torch.randn(2, 256)
    mean = [torch.randn(1, 256) * 0.1]
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=2)
    tr = torch.rand(2, res, res)
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z], None, 0.7, mean, False)[0]
        want = g.renderer.render_surface(ext, focal, near, far, lat, t_rand=tr, refine_steps=3,
                                         want=ALL)
        got = g.render_surface([z], ext, focal, near, far, truncation=0.7,
                               truncation_latent=mean, t_rand=tr, refine_steps=3, want=ALL)
    assert 0 < float(want.hit.sum()) and float(want.normal.abs().max()) > 0
    assert isinstance(got, sdfr.Surface)
    for key in ALL:
        assert torch.equal(getattr(got, key), getattr(want, key)), key


def test_shade_surface_on_a_hand_made_surface(sdfr):
    """5d. hit albedo (ambient + (1 - ambient) max(0, n . l)) with l the unit light vector."""
    hit = torch.tensor([[[[1.0, 1.0], [0.0, 1.0]]]])
    normal = torch.zeros(1, 3, 2, 2)
    normal[0, :, 0, 0] = torch.tensor([0.0, 0.0, 1.0])       # facing the light's z
    normal[0, :, 0, 1] = torch.tensor([0.0, 0.0, -1.0])      # facing away: ambient only
    normal[0, :, 1, 0] = torch.tensor([0.0, 1.0, 0.0])       # a miss: black whatever n is
    normal[0, :, 1, 1] = torch.tensor([0.0, 1.0, 0.0])
    rgb = torch.full((1, 3, 2, 2), 0.5)
    none = [None] * 8
    s = sdfr.Surface(*none)._replace(hit=hit, normal=normal, rgb=rgb)
    light = np.array([-0.5, 1.0, 5.0])
    lz, ly = light[2] / np.linalg.norm(light), light[1] / np.linalg.norm(light)
    img = sdfr.shade_surface(s)
    assert img.shape == (1, 3, 2, 2)
    want = torch.tensor([[0.5 * (0.3 + 0.7 * lz), 0.5 * 0.3], [0.0, 0.5 * (0.3 + 0.7 * ly)]])
    for c in range(3):
        torch.testing.assert_close(img[0, c], want.float(), rtol=0, atol=1e-6)
    white = sdfr.shade_surface(s._replace(rgb=None), light_dir=(0, 0, 2), ambient=0.0)
    torch.testing.assert_close(white[0, 0], torch.tensor([[1.0, 0.0], [0.0, 0.0]]), rtol=0,
                               atol=1e-6)
    grey = sdfr.shade_surface(s, albedo=torch.full((1, 1, 2, 2), 0.25), ambient=1.0)
    torch.testing.assert_close(grey, 0.25 * hit.expand(1, 3, 2, 2), rtol=0, atol=0)
    with pytest.raises(ValueError, match="hit and normal"):
        sdfr.shade_surface(s._replace(normal=None))

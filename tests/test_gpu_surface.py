"""GPU: the fused surface render (sdfr_render_ngp_surface, sdfr_render_siren_surface,
VolumeFeatureRenderer.render_surface) against the fused render's own SDF (bit for bit), a
reference loop over the public query call (depth bit for bit), the gradient and query calls
at the returned points, the op-by-op path on shapes that can break the kernels, and itself
(bands of rows, single outputs, repeated runs)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import weights as W
from tests.test_gpu_render import DEV, _inputs, make_renderer, make_siren
from tests.test_surface import numpy_bracket, surface_layout

pytestmark = pytest.mark.gpu

MAPS = ("hit", "sample", "depth", "xyz", "normal", "rgb", "residual")
ALL = MAPS + ("sdf",)
EPS = 2.0 ** -23
F32 = np.float32

NGP_MESH = dict(static_viewdirs=True, force_background=True, perturb=0)
FIXTURES = [
    ("ngp", "render_mesh_opts", NGP_MESH),
    ("ngp", "render_face64", {}),
    ("siren", "render_siren_mesh_opts", NGP_MESH),
    ("siren", "render_siren_face32", {}),
]
IDS = [f[1] for f in FIXTURES]
# mean |residual| over the hit rays at refine_steps = 8, measured on MI355X
# (profiles/surface_parity.json "surface:<fixture>:residual", [mean K=0, mean K=8, max K=8]);
# seeded inputs and deterministic kernels, so 3x the measured value is a regression tripwire.
# Measured: render_mesh_opts 5.064e-2 -> 1.616e-3 (max 1.049e-2), render_face64 4.772e-2 ->
# 1.955e-3 (max 1.658e-2), render_siren_mesh_opts 9.182e-3 -> 3.818e-7 (max 1.492e-6),
# render_siren_face32 1.163e-2 -> 5.105e-7 (max 3.185e-6).  On the SIREN the floor is the
# fp32 field's own evaluation error at the crossing.  The golden ngp weights give a field
# that is noise along a ray (a random hash table at cells down to 1/4096 of the box), so the
# final bracket of eight halvings (4e-5 in z) still spans several cells and the linear
# interpolation inside it leaves 2e-3.
MEASURED_RESIDUAL = {"render_mesh_opts": 1.616e-3, "render_face64": 1.955e-3,
                     "render_siren_mesh_opts": 3.818e-7, "render_siren_face32": 5.105e-7}

_record = {}


def teardown_module(module):
    out = os.environ.get("SDFR_PARITY_JSON")
    if out:
        prev = {}
        if os.path.exists(out):
            with open(out) as f:
                prev = json.load(f)
        prev.update(_record)
        with open(out, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def state_dicts(golden_dir):
    return {"ngp": W.det_state_dict(W.golden_entries(golden_dir), "renderer."),
            "siren": W.det_state_dict(W.golden_entries(golden_dir, siren=True), "renderer.")}


def _make(sdfr, state_dicts, net, res, N, **flags):
    make = make_renderer if net == "ngp" else make_siren
    return make(sdfr, state_dicts[net], res, N, return_sdf=True, **flags)


def _surface(ren, inputs, **kw):
    cam, focal, near, far, lat, tr = inputs
    with torch.no_grad():
        assert ren._query_fused_ok(cam, lat)
        return ren.render_surface(cam, focal, near, far, lat, t_rand=tr, **kw)


def _module_surface(ren, inputs, **kw):
    cam, focal, near, far, lat, tr = inputs
    ren.use_fused = False
    try:
        assert not ren._query_fused_ok(cam, lat)
        with torch.no_grad():
            return ren.render_surface(cam, focal, near, far, lat, t_rand=tr, **kw)
    finally:
        ren.use_fused = True


_CASES = {}


def _case(sdfr, golden_dir, state_dicts, oracle_mod, net, name, flags):
    """The fixture's renderer, inputs, the oracle's rays and the K = 8 surface, shared by
    the tests of a fixture (none of them changes it)."""
    if name not in _CASES:
        g = np.load(golden_dir / f"{name}.npz")
        ren = _make(sdfr, state_dicts, net, int(g["res"]), int(g["n_samples"]), **flags)
        inputs = _inputs(g)
        tr = g["t_rand"] if ren.perturb > 0 and np.size(g["t_rand"]) else None
        ray = oracle_mod.sample_rays(g["ext"], g["focal"], g["near"], g["far"], ren.out_im_res,
                                     ren.out_im_res, ren.N_samples, t_rand=tr,
                                     offset_sampling=ren.offset_sampling,
                                     static_viewdirs=bool(ren.static_viewdirs),
                                     z_normalize=ren.z_normalize)
        _CASES[name] = (g, ren, inputs, ray, _surface(ren, inputs, want=ALL))
    return _CASES[name]


def _network_coords(p, g, z_normalize):
    """p [B,..,3] world (fp32) -> the network coordinate by the definition's rounded ops."""
    if not z_normalize:
        return p
    B = p.shape[0]
    span = (g["far"].astype(F32) - g["near"].astype(F32)).reshape((B,) + (1,) * (p.ndim - 1))
    return ((p * F32(2)) / span).astype(F32)


def _origins(g, like):
    B = like.shape[0]
    o = g["ext"].astype(F32).reshape(B, 3, 4)[:, :, 3]
    return np.broadcast_to(o.reshape((B,) + (1,) * (like.ndim - 2) + (3,)), like.shape)


@pytest.mark.parametrize("net,name,flags", FIXTURES, ids=IDS)
def test_coarse_sdf_is_the_render_and_bracket_is_exact(sdfr, golden_dir, state_dicts, oracle_mod,
                                                       net, name, flags):
    """6. sdf is the fused render's return_sdf bit for bit; hit and sample are the numpy
    bracket of that sdf exactly.  The ngp fixtures have hit and miss rays."""
    g, ren, inputs, _, surf = _case(sdfr, golden_dir, state_dicts, oracle_mod, net, name, flags)
    cam, focal, near, far, lat, tr = inputs
    with torch.no_grad():
        assert ren._fused_ok(cam, lat, False)
        sdf_r = ren.fused_forward(cam, focal, near, far, lat, t_rand=tr)[2]
    assert surf.sdf.shape == sdf_r.shape and torch.equal(surf.sdf, sdf_r)
    hit, s = numpy_bracket(surf.sdf[..., 0].cpu().numpy())
    assert np.array_equal(surf.hit[:, 0].cpu().numpy(), hit.astype(F32))
    assert np.array_equal(surf.sample[:, 0].cpu().numpy(), s)
    frac = float(hit.mean())
    _record[f"surface:{name}:hit_fraction"] = frac
    print(f"{name}: {frac:.3f} of the rays cross")
    if net == "ngp":
        assert hit.any() and not hit.all()
    else:
        assert hit.all()
    for key in ("depth", "xyz", "normal", "rgb", "residual"):
        v = getattr(surf, key).permute(0, 2, 3, 1).cpu().numpy()
        assert (v[~hit] == 0).all() and np.isfinite(v).all(), key


def _reference_depth(ren, g, ray, sdf, lat, steps):
    """The definition in numpy fp32, one rounded operation per step, the SDF of every
    midpoint from the public query call.  Returns depth [B,H,W] (0 on a miss)."""
    B, H, Wd, N = sdf.shape
    hit, s = numpy_bracket(sdf)
    s0 = np.where(hit, s, 0)[..., None].astype(np.int64)
    s1 = np.minimum(s0 + 1, N - 1)
    z = ray["z_vals"].astype(F32)
    a, b = np.take_along_axis(z, s0, -1)[..., 0], np.take_along_axis(z, s1, -1)[..., 0]
    fa, fb = np.take_along_axis(sdf, s0, -1)[..., 0], np.take_along_axis(sdf, s1, -1)[..., 0]
    d = ray["rays_d"].astype(F32)
    o = _origins(g, d)
    for _ in range(steps):
        m = F32(0.5) * (a + b)
        p = o + d * m[..., None]
        pn = _network_coords(p, g, ren.z_normalize)
        with torch.no_grad():
            f, _ = ren.query(torch.from_numpy(pn.reshape(B, -1, 3)).to(DEV), lat,
                             return_rgb=False)
        f = f.cpu().numpy().reshape(B, H, Wd)
        pos = f > 0
        a, fa = np.where(pos, m, a), np.where(pos, f, fa)
        b, fb = np.where(pos, b, m), np.where(pos, fb, f)
    with np.errstate(divide="ignore", invalid="ignore"):
        zs = a + (fa / (fa - fb)) * (b - a)
    zs = np.minimum(np.maximum(zs, a), b)
    assert zs.dtype == F32
    return np.where(hit, zs, F32(0)), hit, b - a


@pytest.mark.parametrize("steps", [0, 1, 8])
@pytest.mark.parametrize("net,name,flags", FIXTURES, ids=IDS)
def test_depth_equals_a_loop_over_the_query_call(sdfr, golden_dir, state_dicts, oracle_mod, net,
                                                 name, flags, steps):
    """7. depth bit for bit against the definition written out in numpy fp32 with
    renderer.query(return_rgb=False) for every bisection step."""
    g, ren, inputs, ray, surf8 = _case(sdfr, golden_dir, state_dicts, oracle_mod, net, name, flags)
    surf = surf8 if steps == 8 else _surface(ren, inputs, refine_steps=steps,
                                             want=("depth", "sdf"))
    want, hit, width = _reference_depth(ren, g, ray, surf.sdf[..., 0].cpu().numpy(), inputs[4],
                                        steps)
    got = surf.depth[:, 0].cpu().numpy()
    diff = np.abs(got.astype(np.float64) - want)
    print(f"{name} K={steps}: max |depth - loop| {diff.max():.3e}, "
          f"final bracket width up to {float(width[hit].max()):.3e}")
    assert np.array_equal(got, want)


def _raw_surface(sdfr, ren, net, inputs, steps):
    """The C entry point itself on a whole call with NaN-filled outputs and no prepacked
    weights (the call packs inside its workspace): the Surface and the workspace."""
    cam, focal, near, far, lat, tr = inputs
    B, H, N = cam.shape[0], ren.out_im_res, ren.N_samples
    L = sdfr._lib.lib()
    cam, focal, near, far, lat, tr, per_sample, pix_x, pix_y, t_vals = \
        ren._fused_inputs(cam, focal, near, far, lat, tr)
    out = {k: torch.full((B, 3 if k in ("xyz", "normal", "rgb") else 1, H, H), float("nan"),
                         device=DEV) for k in MAPS if k != "sample"}
    out["sample"] = torch.full((B, 1, H, H), -7, dtype=torch.int32, device=DEV)
    out["sdf"] = torch.full((B, H, H, N), float("nan"), device=DEV)
    need = getattr(L, f"sdfr_render_{net}_surface_workspace_bytes")(B, H, H, N)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ptr = sdfr._lib.ptr
    a = sdfr._lib.SurfaceArgs(
        B=B, H=H, W=H, N=N, cam=ptr(cam), focal=ptr(focal), near_=ptr(near), far_=ptr(far),
        styles=ptr(lat), pix_x=ptr(pix_x), pix_y=ptr(pix_y), t_vals=ptr(t_vals), t_rand=ptr(tr),
        t_rand_per_sample=per_sample, offset_sampling=int(ren.offset_sampling),
        static_viewdirs=int(bool(ren.static_viewdirs)), z_normalize=int(ren.z_normalize),
        refine_steps=steps, workspace=ptr(ws), workspace_bytes=ws.numel(), prepacked=None,
        prepacked_grad=None, **{k: ptr(v) for k, v in out.items()})
    w = ren._weight_struct(0 if net == "ngp" else 1)
    fn = f"sdfr_render_{net}_surface"
    sdfr._lib.check(getattr(L, fn)(ctypes.byref(w), ctypes.byref(a), sdfr._lib.stream_of(cam)), fn)
    torch.cuda.synchronize()
    out["sdf"] = out["sdf"].unsqueeze(-1)
    return sdfr.Surface(**out), ws


@pytest.mark.parametrize("net,name,flags", FIXTURES, ids=IDS)
def test_values_at_the_hit_are_the_public_calls(sdfr, golden_dir, state_dicts, oracle_mod, net,
                                                name, flags):
    """8. At the returned xyz (in network coordinates by the definition's ops): residual is
    query_gradient's SDF bit for bit, normal its scaled gradient normalised to 16 eps per
    component, rgb is query's colour with the per-ray directions bit for bit, and xyz is
    o + d depth in the rounded ops.
    The per-ray directions are the render's: v / |v| with the device's square root, which
    is within one ulp of the correctly rounded one and so differs from the oracle's
    direction in the last bit on a few rays per thousand.  The test therefore takes them
    from the call's own workspace (the region the header documents), holds them to the
    oracle's within 2 ulp, and holds rgb to the query call at exactly those directions.
    The raw call packs the weights inside its workspace; every output equals the Python
    path's, which passes prepacked weights."""
    g, ren, inputs, ray, surf = _case(sdfr, golden_dir, state_dicts, oracle_mod, net, name, flags)
    raw, ws = _raw_surface(sdfr, ren, net, inputs, 8)
    for key in ALL:
        assert torch.equal(getattr(raw, key), getattr(surf, key)), key
    Bn, Hn, Nn = inputs[0].shape[0], ren.out_im_res, ren.N_samples
    off = surface_layout(sdfr._lib.lib(), net, Bn, Hn, Hn, Nn)
    assert off["total"] == ws.numel()
    nd = Bn * Hn * Hn * 3
    dirs = ws[off["directions"]:off["directions"] + 4 * nd].view(torch.float32).view(Bn, -1, 3)
    want_dirs = ray["viewdirs"].astype(F32).reshape(Bn, -1, 3)
    assert float(np.abs(dirs.cpu().numpy() - want_dirs).max()) <= 2 * EPS
    lat = inputs[4]
    hit = surf.hit[:, 0].cpu().numpy() > 0
    B, H, Wd = hit.shape
    d = ray["rays_d"].astype(F32)
    depth = surf.depth[:, 0].cpu().numpy()
    xyz = surf.xyz.permute(0, 2, 3, 1).cpu().numpy()
    want_xyz = _origins(g, d) + d * depth[..., None]
    assert np.array_equal(xyz[hit], want_xyz[hit])
    pn = torch.from_numpy(_network_coords(xyz, g, ren.z_normalize).reshape(B, -1, 3)).to(DEV)
    with torch.no_grad():
        sdf_g, grad = ren.query_gradient(pn, lat)
        _, rgb_q = ren.query(pn, lat, viewdirs=dirs.clone())
    res = surf.residual[:, 0].cpu().numpy()
    assert np.array_equal(res[hit], sdf_g.cpu().numpy().reshape(B, H, Wd)[hit])
    e = grad.double()
    if ren.z_normalize:
        span = (inputs[3].reshape(B, 1, 1) - inputs[2].reshape(B, 1, 1)).double()
        e = e * 2 / span
    unit = (e / e.norm(dim=-1, keepdim=True).clamp_min(1e-20)).cpu().numpy().reshape(B, H, Wd, 3)
    nrm = surf.normal.permute(0, 2, 3, 1).cpu().numpy()
    err = float(np.abs(nrm[hit] - unit[hit]).max())
    _record[f"surface:{name}:normal_vs_gradient_call"] = err
    assert err <= 16 * EPS
    assert np.abs(np.linalg.norm(nrm[hit].astype(np.float64), axis=-1) - 1).max() <= 4 * EPS
    rgb = surf.rgb.permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(rgb[hit], rgb_q.cpu().numpy().reshape(B, H, Wd, 3)[hit])
    assert rgb[hit].min() >= 0 and rgb[hit].max() <= 1 and rgb[hit].max() > 0


@pytest.mark.parametrize("net,name,flags", FIXTURES, ids=IDS)
def test_refinement_shrinks_the_residual(sdfr, golden_dir, state_dicts, oracle_mod, net, name,
                                         flags):
    """9. Mean |residual| over the hit rays at K = 8 is strictly below K = 0's; the K = 8
    value stays within 3x of the one measured on MI355X."""
    _, ren, inputs, _, surf8 = _case(sdfr, golden_dir, state_dicts, oracle_mod, net, name, flags)
    surf0 = _surface(ren, inputs, refine_steps=0, want=("hit", "residual"))
    assert torch.equal(surf0.hit, surf8.hit)
    hit = surf8.hit > 0
    m0 = float(surf0.residual[hit].abs().mean())
    m8 = float(surf8.residual[hit].abs().mean())
    x8 = float(surf8.residual[hit].abs().max())
    _record[f"surface:{name}:residual"] = [m0, m8, x8]
    print(f"{name}: mean |residual| K=0 {m0:.3e} K=8 {m8:.3e} (max {x8:.3e})")
    assert m8 < m0
    measured = MEASURED_RESIDUAL[name]
    assert measured is not None and m8 <= 3 * measured


def _cameras(sdfr, res, B, seed):
    torch.manual_seed(seed)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.from_numpy(W.det_uniform((B, 256), -1.5, 1.5, 5 + seed))
    tr = torch.rand(B, res, res)
    return [t.to(DEV) for t in (ext, focal, near, far, lat)] + [tr]


SHAPES = [(1, 5, 3), (2, 3, 1), (2, 3, 2), (1, 3, 130), (2, 8, 24)]


@pytest.mark.parametrize("net", ["ngp", "siren"])
@pytest.mark.parametrize("B,res,N", SHAPES)
def test_shapes_vs_module_path(sdfr, state_dicts, net, B, res, N):
    """10. 25 rays (a partial group of 32 and a partial tile of 16), one and two samples per
    ray, N = 130 (three 64-lane chunks of the bracket kernel, with a crossing between
    samples 63 and 64) and two faces with different latents: hit and sample exact against
    the numpy bracket of the call's own sdf, depth within one final-bracket width of the
    op-by-op path's."""
    ren = _make(sdfr, state_dicts, net, res, N)
    inputs = _cameras(sdfr, res, B, 100 * res + N)
    K = 8
    if N == 130:
        # Shift the SDF (sigma_linear.bias) so that some ray's first crossing lies between
        # samples 63 and 64: a ray whose sample 64 is below all its samples 0..63 (the golden
        # ngp weights give an SDF that is noise along a ray, so that is one ray in 65), and a
        # level a quarter of the way up from sample 64 to the lowest of them.  The cameras
        # and latents are tried in seed order until a ray has one; the choice looks at the
        # coarse SDF only.
        shift = None
        for seed in range(64):
            inputs = _cameras(sdfr, res, B, 100 * res + N + seed)
            base = _surface(ren, inputs, want=("sdf",)).sdf[..., 0].cpu().numpy().reshape(-1, N)
            for row in base:
                t = -(0.75 * float(row[64]) + 0.25 * float(row[:64].min()))
                if row[:64].min() > row[64] and numpy_bracket(row + F32(t))[1] == 63:
                    shift = t
                    break
            if shift is not None:
                break
        assert shift is not None, "no ray can put its first crossing at sample 63"
        with torch.no_grad():
            ren.network.sigma_linear.bias += shift
    fused = _surface(ren, inputs, refine_steps=K, want=ALL)
    mod = _module_surface(ren, inputs, refine_steps=K, want=ALL)
    sdf = fused.sdf[..., 0].cpu().numpy()
    hit, s = numpy_bracket(sdf)
    assert np.array_equal(fused.hit[:, 0].cpu().numpy(), hit.astype(F32))
    assert np.array_equal(fused.sample[:, 0].cpu().numpy(), s)
    if N == 1:
        assert not hit.any()
    if N == 130:
        assert (s == 63).any(), "no crossing across the 64-lane chunk boundary"
    if B == 2 and N > 1:
        assert not torch.equal(fused.sdf[0], fused.sdf[1])
    for v in fused:
        assert not v.requires_grad and torch.isfinite(v.float()).all()
    # The op-by-op path evaluates the field in plain fp32, so a sample within rounding of
    # zero may give it another bracket: the depths are compared where the two paths chose
    # the same one.  There they agree within the final bracket's width: one ray's offset
    # shifts all its samples alike, so the spacing is (far - near) / N, halved K times
    # (plus the rounding of z itself, a few ulp of far).
    same = torch.from_numpy(hit).to(DEV) & (mod.sample[:, 0] == fused.sample[:, 0])
    if hit.any():
        assert same.any()
        near, far = inputs[2].reshape(B, 1, 1), inputs[3].reshape(B, 1, 1)
        width = (far - near) / N / 2 ** K + 4 * EPS * far
        err = (fused.depth[:, 0] - mod.depth[:, 0]).abs()
        print(f"{net} B={B} res={res} N={N}: {int(hit.sum())} hits, max depth diff "
              f"{float(err[same].max()):.3e} (width {float(width.max()):.3e})")
        assert (err[same] <= width.expand_as(err)[same]).all()


@pytest.mark.parametrize("net", ["ngp", "siren"])
def test_bands_single_outputs_and_repeats_are_bitwise_neutral(sdfr, state_dicts, net):
    """11. B = 3, 8 x 8 x 24: one-row bands, a few rows per band, one face per call and
    single outputs (the null-pointer combinations) equal the single call's bits; two runs
    are equal; weights with no zero crossing give zeros."""
    B, res, N = 3, 8, 24
    ren = _make(sdfr, state_dicts, net, res, N)
    inputs = _cameras(sdfr, res, B, 7)
    one = _surface(ren, inputs, want=ALL)
    assert 0 < float(one.hit.sum()) and one.normal.abs().max() > 0 and one.rgb.max() > 0
    again = _surface(ren, inputs, want=ALL)
    for key in ALL:
        assert torch.equal(getattr(again, key), getattr(one, key)), key
    for chunk in (1, 3 * res * N + 5, res * res * N):
        got = _surface(ren, inputs, want=ALL, chunk_points=chunk)
        for key in ALL:
            assert torch.equal(getattr(got, key), getattr(one, key)), (chunk, key)
    for key in ALL:
        got = _surface(ren, inputs, want=(key,), chunk_points=3 * res * N)
        assert [k for k in ALL if getattr(got, k) is not None] == [key]
        assert torch.equal(getattr(got, key), getattr(one, key)), key
    # stratified sampling: t_rand is per sample, [B,H,W,N]
    ren2 = _make(sdfr, state_dicts, net, res, N, no_offset_sampling=True)
    in2 = inputs[:5] + [torch.rand(B, res, res, N)]
    one2 = _surface(ren2, in2, want=ALL)
    got2 = _surface(ren2, in2, want=ALL, chunk_points=3 * res * N)
    with torch.no_grad():
        sdf_r = ren2.fused_forward(*in2[:5], t_rand=in2[5])[2]
    assert torch.equal(one2.sdf, sdf_r)
    for key in ALL:
        assert torch.equal(getattr(got2, key), getattr(one2, key)), key
    for shift in (1.0, -2.0):                # all outside, all inside: no outside -> inside
        with torch.no_grad():
            ren.network.sigma_linear.bias += shift
        miss = _surface(ren, inputs, want=MAPS)
        with torch.no_grad():
            ren.network.sigma_linear.bias -= shift
        assert (miss.sample == -1).all()
        for key in MAPS:
            if key != "sample":
                assert (getattr(miss, key) == 0).all(), (shift, key)

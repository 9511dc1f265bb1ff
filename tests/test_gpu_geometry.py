"""GPU: the fused geometry render (sdfr_render_ngp_geometry,
VolumeFeatureRenderer.render_geometry) against the reference's eikonal fixture, the fused
render's own SDF (bit for bit), the gradient call at the same points, the reference's xyz /
mask maps, float64 composites, and the op-by-op path on shapes that can break the kernels."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import weights as W
from tests.test_gpu_query_gradient import RATIO, _ref64
from tests.test_gpu_render import DEV, TOL, _inputs, make_renderer
from tests.test_gpu_stage1 import _stage1_generator

pytestmark = pytest.mark.gpu

ALL = ("normal", "depth", "xyz", "mask", "sdf", "eikonal")
MAPS = ("normal", "depth", "xyz", "mask")
# the project's relative bounds (of the tensor's largest magnitude) for the eikonal term
# and the per-sample SDF against the reference's fixtures (tests/test_gpu_stage1.py)
REL_EIKONAL, REL_SDF = 1e-4, 2e-5
# z-normalisation scales the network-coordinate gradient by two correctly rounded
# operations (fmul by 2, exact; fdiv by far - near): 4 ulp relative
ULP4 = 4 * 2.0 ** -23
# max |map - float64 composite of the call's own fp32 sdf / eikonal|: 3x the value measured
# on MI355X (profiles/geometry_parity.json "geometry:<fixture>:normal64" / ":depth64", [max
# error, largest |map|]); seeded inputs and deterministic kernels, so a regression tripwire.
# normal 3.237e-4 at max |normal| 1116 (render_face64; render_mesh_opts 2.345e-4 at 914), depth
# 3.819e-7 at 1.05 (render_face64; render_mesh_opts 1.823e-7).
MEASURED64 = {"normal": 3.237e-4, "depth": 3.819e-7}
TOL64 = {k: 3 * v for k, v in MEASURED64.items()}

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
def renderer_sd(golden_dir):
    return W.det_state_dict(W.golden_entries(golden_dir), "renderer.")


def _rel(got, ref):
    """max |got - ref| / max |ref|, and the mean error on the same scale."""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    ref = np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref)
    return float(err.max()) / scale, float(err.mean()) / scale


def _geo(ren, cam, focal, near, far, lat, tr, want=ALL, **kw):
    with torch.no_grad():
        assert ren._query_fused_ok(cam, lat)
        return ren.render_geometry(cam, focal, near, far, lat, t_rand=tr, want=want, **kw)


def _module_geo(ren, cam, focal, near, far, lat, tr, want=ALL):
    """The op-by-op path on the GPU (autograd through renderer.network)."""
    ren.use_fused = False
    try:
        assert not ren._query_fused_ok(cam, lat)
        return ren.render_geometry(cam, focal, near, far, lat, t_rand=tr, want=want)
    finally:
        ren.use_fused = True


def _oracle_rays(oracle_mod, g, ren):
    res, N = ren.out_im_res, ren.N_samples
    tr = g["t_rand"] if ren.perturb > 0 and np.size(g["t_rand"]) else None
    return oracle_mod.sample_rays(g["ext"], g["focal"], g["near"], g["far"], res, res, N,
                                  t_rand=tr, offset_sampling=ren.offset_sampling,
                                  static_viewdirs=bool(ren.static_viewdirs),
                                  z_normalize=ren.z_normalize)


def _maps64(sdf, eik, ray, beta, force_background):
    """normal / depth / xyz / mask [B,H,W,C] in float64 from per-sample sdf [B,H,W,N] and
    eikonal [B,H,W,N,3]: the reference's weight formula (sdf_model.py:236-301) on its own
    fp32 segment lengths (z differences and |d| as the reference rounds them)."""
    z32, dn32 = ray["z_vals"], ray["dnorm"][..., None]
    dists = np.concatenate([z32[..., 1:] - z32[..., :-1],
                            np.full_like(z32[..., :1], 1e10)], -1) * dn32
    assert dists.dtype == np.float32
    sdf, dists, z = np.asarray(sdf, np.float64), dists.astype(np.float64), z32.astype(np.float64)
    sigma = 1.0 / (1.0 + np.exp(sdf / beta)) / beta                  # sigmoid(-sdf / beta) / beta
    alpha = 1 - np.exp(-sigma * dists)
    T = np.cumprod(np.concatenate([np.ones_like(alpha[..., :1]), 1 - alpha + 1e-10], -1),
                   -1)[..., :-1]
    w = alpha * T
    if force_background:
        w[..., -1] = 1 - w[..., :-1].sum(-1)
    return dict(normal=(w[..., None] * np.asarray(eik, np.float64)).sum(3),
                depth=(w * z).sum(-1)[..., None],
                xyz=(w[..., None] * ray["pts"].astype(np.float64)).sum(3),
                mask=w[..., -1:])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).cpu().numpy()


def _network_points(ray, g, z_normalize):
    """The samples' network coordinates as the kernels round them (x 2, / (far - near))."""
    B = ray["pts"].shape[0]
    if not z_normalize:
        return ray["pts"].reshape(B, -1, 3)
    span = (g["far"] - g["near"]).reshape(B, 1, 1, 1, 1).astype(np.float32)
    return ((ray["pts"] * np.float32(2)) / span).astype(np.float32).reshape(B, -1, 3)


# --------------------------------------------------------------------------------------
def test_eikonal_vs_reference_golden(sdfr, golden_dir, oracle_mod):
    """5. eikonal.npz: the fused eikonal term and SDF against the reference's own, with the
    project's relative bounds, and the eikonal error at most 3x the op-by-op path's
    (forward(return_eikonal=True)) against the same golden.  Samples outside the grid's
    box are exactly zero."""
    g = np.load(golden_dir / "eikonal.npz")
    gen = _stage1_generator(sdfr, golden_dir, g)
    t = lambda k: torch.from_numpy(g[k]).to(DEV)  # noqa: E731
    tr = torch.from_numpy(g["t_rand"])
    with torch.no_grad():
        geo = gen.render_geometry([t("z")], t("ext"), t("focal"), t("near"), t("far"),
                                  t_rand=tr, want=("sdf", "eikonal"))
    assert geo.normal is None and geo.mask is None
    assert geo.sdf.shape == g["sdf"].shape and geo.eikonal.shape == g["eikonal"].shape
    assert not geo.eikonal.requires_grad
    _, _, sdf_m, eik_m = gen([t("z")], t("ext"), t("focal"), t("near"), t("far"),
                             return_sdf=True, return_eikonal=True, t_rand=tr)
    ef, ef_mean = _rel(geo.eikonal.cpu(), g["eikonal"])
    em, em_mean = _rel(eik_m.detach().cpu(), g["eikonal"])
    sf, _ = _rel(geo.sdf.cpu(), g["sdf"])
    sm, _ = _rel(sdf_m.detach().cpu(), g["sdf"])
    scale = float(np.abs(g["eikonal"]).max())
    _record["geometry:eikonal_golden:eikonal"] = [ef, ef_mean, scale]
    _record["geometry:eikonal_golden:eikonal_module"] = [em, em_mean, scale]
    _record["geometry:eikonal_golden:sdf"] = [sf, sm]
    print(f"eikonal vs golden: fused {ef:.3e} (mean {ef_mean:.3e}) module {em:.3e} "
          f"(mean {em_mean:.3e}) of max |ref| {scale:.3e}; sdf fused {sf:.3e} module {sm:.3e}")
    assert ef <= REL_EIKONAL and sf <= REL_SDF
    assert ef <= RATIO * em, f"fused eikonal err {ef:.3e} > {RATIO} x module {em:.3e}"
    ray = _oracle_rays(oracle_mod, g, gen.renderer)
    outside = ((ray["grid_in"] < 0) | (ray["grid_in"] > 1)).any(-1)
    _record["geometry:eikonal_golden:outside"] = int(outside.sum())
    eik = geo.eikonal.cpu().numpy()
    assert (eik[outside] == 0).all() and (g["eikonal"][outside] == 0).all()
    assert np.abs(eik[~outside]).max() > 0


BIT_CASES = [
    ("render_small", {}),
    ("render_mesh_opts", dict(static_viewdirs=True, force_background=True, perturb=0)),
]


@pytest.mark.parametrize("name,flags", BIT_CASES)
def test_sdf_bit_identical_to_render_and_gradient_call(sdfr, golden_dir, oracle_mod,
                                                       renderer_sd, name, flags):
    """6. The per-sample SDF is the fused render's return_sdf output and the gradient
    call's SDF at the same points, bit for bit; the eikonal term is the gradient call's
    gradient (equal without z-normalisation, times 2 / (far - near) within 4 ulp with it)."""
    g = np.load(golden_dir / f"{name}.npz")
    res, N = int(g["res"]), int(g["n_samples"])
    cam, focal, near, far, lat, tr = _inputs(g)
    B = cam.shape[0]
    for extra in ({}, dict(no_z_normalize=True)):
        ren = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True, **flags, **extra)
        geo = _geo(ren, cam, focal, near, far, lat, tr, want=("sdf", "eikonal"))
        with torch.no_grad():
            assert ren._fused_ok(cam, lat, False)
            sdf_r = ren.fused_forward(cam, focal, near, far, lat, t_rand=tr)[2]
        assert geo.sdf.shape == (B, res, res, N, 1) == sdf_r.shape
        assert torch.equal(geo.sdf, sdf_r)
        ray = _oracle_rays(oracle_mod, g, ren)
        tp = torch.from_numpy(_network_points(ray, g, ren.z_normalize)).to(DEV)
        with torch.no_grad():
            sdf_q, grad_q = ren.query_gradient(tp, lat)
        assert torch.equal(geo.sdf.reshape(B, -1), sdf_q)
        grad_q = grad_q.view(B, res, res, N, 3)
        assert grad_q.abs().max() > 0
        if not ren.z_normalize:
            assert torch.equal(geo.eikonal, grad_q)
        else:
            span = (far.reshape(B, 1, 1, 1, 1) - near.reshape(B, 1, 1, 1, 1)).double()
            want = grad_q.double() * 2 / span
            rel = ((geo.eikonal.double() - want).abs() / want.abs().clamp_min(1e-300)).max()
            _record[f"geometry:{name}:eikonal_scale_ulp"] = float(rel) / 2.0 ** -23
            assert float(rel) <= ULP4
            assert ((geo.eikonal == 0) == (grad_q == 0)).all()


@pytest.mark.parametrize("name,flags", [
    ("render_mesh_opts", dict(static_viewdirs=True, force_background=True, perturb=0)),
    ("render_face64", {}),
])
def test_maps_vs_reference_and_float64_composite(sdfr, golden_dir, oracle_mod, renderer_sd,
                                                 name, flags):
    """7. xyz / mask against the reference's (the render's bounds: the formulas are the
    render's); normal / depth against a float64 composite of the call's own fp32 sdf and
    eikonal with the oracle's z-values and the reference's weight formula."""
    g = np.load(golden_dir / f"{name}.npz")
    res, N = int(g["res"]), int(g["n_samples"])
    ren = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True, return_xyz=True, **flags)
    cam, focal, near, far, lat, tr = _inputs(g)
    geo = _geo(ren, cam, focal, near, far, lat, tr)
    B = cam.shape[0]
    assert geo.normal.shape == (B, 3, res, res) and geo.depth.shape == (B, 1, res, res)
    for key in ("xyz", "mask"):
        err = np.abs(getattr(geo, key).cpu().numpy().astype(np.float64) - g[key])
        _record[f"geometry:{name}:{key}"] = [float(err.max()), float(err.mean())]
        print(f"{name}:{key} max {err.max():.3e} mean {err.mean():.3e} (bounds {TOL[key]})")
    for key in ("xyz", "mask"):
        emax, emean = _record[f"geometry:{name}:{key}"]
        assert emax <= TOL[key][0], f"{name}:{key} max err {emax:.3e} > {TOL[key][0]:.1e}"
        assert emean <= TOL[key][1], f"{name}:{key} mean err {emean:.3e} > {TOL[key][1]:.1e}"
    with torch.no_grad():                                   # and the fused render's own
        out = ren.fused_forward(cam, focal, near, far, lat, t_rand=tr)
    assert torch.equal(geo.sdf, out[2])
    ray = _oracle_rays(oracle_mod, g, ren)
    ref = _maps64(geo.sdf[..., 0].cpu().numpy(), geo.eikonal.cpu().numpy(), ray,
                  float(ren.sigmoid_beta.detach()), bool(ren.force_background))
    for key in MAPS:
        got = _nhwc(getattr(geo, key)).astype(np.float64)
        err, scale = float(np.abs(got - ref[key]).max()), float(np.abs(ref[key]).max())
        _record[f"geometry:{name}:{key}64"] = [err, scale]
        print(f"{name}:{key} vs float64 composite: max err {err:.3e} at max |map| {scale:.3e}")
    for key in ("normal", "depth"):
        err = _record[f"geometry:{name}:{key}64"][0]
        assert err <= TOL64[key], f"{name}:{key} err {err:.3e} > {TOL64[key]:.2e}"
    # the fused render's xyz / mask use the same expressions (its f16x3 kernel adds two
    # half-sums per ray): the same bounds hold between the two
    for key, idx in (("xyz", 4), ("mask", 3)):
        d = (getattr(geo, key) - out[idx]).abs()
        assert float(d.max()) <= TOL[key][0]
    n = _geo(ren, cam, focal, near, far, lat, tr, want=("normal",), normalize=True).normal
    assert torch.equal(n, geo.normal / geo.normal.norm(dim=1, keepdim=True).clamp_min(1e-20))
    torch.testing.assert_close(n.norm(dim=1), torch.ones(B, res, res, device=DEV), rtol=0,
                               atol=1e-6)


def _cameras(sdfr, res, B, seed):
    torch.manual_seed(seed)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.from_numpy(W.det_uniform((B, 256), -1.5, 1.5, 5 + seed))
    tr = torch.rand(B, res, res)
    return [t.to(DEV) for t in (ext, focal, near, far, lat)] + [tr]


@pytest.mark.parametrize("B,res,N", [(2, 5, 3), (2, 8, 1)])
def test_shapes_vs_module_path(sdfr, oracle_mod, renderer_sd, B, res, N):
    """8a. 75 points per face (a partly filled wave and workgroup pass) and one sample per
    ray (the 1e10 last segment only): every output against a float64 reference (the
    oracle's hash-grid values and dy_dx, the SDF trunk in float64, the reference's
    weights), the fused error at most 3x the op-by-op path's."""
    ren = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True)
    cam, focal, near, far, lat, tr = _cameras(sdfr, res, B, 100 * res + N)
    geo = _geo(ren, cam, focal, near, far, lat, tr)
    mod = _module_geo(ren, cam, focal, near, far, lat, tr)
    for v in list(geo) + list(mod):
        assert not v.requires_grad
    g = dict(ext=cam.cpu().numpy(), focal=focal.cpu().numpy(), near=near.cpu().numpy(),
             far=far.cpu().numpy(), t_rand=tr.numpy())
    ray = _oracle_rays(oracle_mod, g, ren)
    npts = _network_points(ray, g, True)
    sdf64, grad64 = _ref64(oracle_mod, renderer_sd, npts, lat.cpu().numpy())
    span = (g["far"] - g["near"]).reshape(B, 1, 1, 1, 1).astype(np.float32).astype(np.float64)
    ref = dict(sdf=sdf64.reshape(B, res, res, N, 1),
               eikonal=grad64.reshape(B, res, res, N, 3) * 2 / span)
    ref.update(_maps64(ref["sdf"][..., 0], ref["eikonal"], ray, float(ren.sigmoid_beta.detach()),
                       False))
    assert np.abs(ref["eikonal"]).max() > 0
    bad = []
    for key in ALL:
        f, m = getattr(geo, key), getattr(mod, key)
        assert f.shape == m.shape
        if key in MAPS:
            f, m = _nhwc(f), _nhwc(m)
        else:
            f, m = f.cpu().numpy(), m.cpu().numpy()
        (ef, ef_mean), (em, em_mean) = _rel(f, ref[key]), _rel(m, ref[key])
        _record[f"geometry:shape_{res}x{N}:{key}"] = [ef, em, ef_mean, em_mean]
        print(f"res {res} N {N} {key}: fused {ef:.3e} module {em:.3e} (relative max; mean "
              f"{ef_mean:.3e} / {em_mean:.3e})")
        if ef > RATIO * em:
            bad.append((key, ef, em))
    assert not bad, f"fused error above {RATIO} x the module path's: {bad}"


def test_bands_of_rows_and_single_outputs_are_bitwise_neutral(sdfr, renderer_sd):
    """8b. B = 3, 8 x 8 x 24 with chunk_points forcing bands of 3 rows (3 + 3 + 2 rows,
    several calls per face, per-band t_rand slices), one face per call, and single
    outputs (the null-pointer combinations): every output equals the single call's."""
    B, res, N = 3, 8, 24
    ren = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True)
    cam, focal, near, far, lat, tr = _cameras(sdfr, res, B, 7)
    one = _geo(ren, cam, focal, near, far, lat, tr)
    assert one.eikonal.abs().max() > 0 and one.normal.abs().max() > 0
    for chunk in (3 * res * N, 3 * res * N + 5, res * res * N, 1):
        got = _geo(ren, cam, focal, near, far, lat, tr, chunk_points=chunk)
        for key in ALL:
            assert torch.equal(getattr(got, key), getattr(one, key)), (chunk, key)
    for key in ("eikonal", "depth", "sdf", "mask"):
        got = _geo(ren, cam, focal, near, far, lat, tr, want=(key,), chunk_points=3 * res * N)
        assert [k for k in ALL if getattr(got, k) is not None] == [key]
        assert torch.equal(getattr(got, key), getattr(one, key)), key
    # stratified sampling: t_rand is per sample, [B,H,W,N]
    ren2 = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True, no_offset_sampling=True)
    tr2 = torch.rand(B, res, res, N)
    one = _geo(ren2, cam, focal, near, far, lat, tr2)
    got = _geo(ren2, cam, focal, near, far, lat, tr2, chunk_points=3 * res * N)
    with torch.no_grad():
        sdf_r = ren2.fused_forward(cam, focal, near, far, lat, t_rand=tr2)[2]
    assert torch.equal(one.sdf, sdf_r)
    for key in ALL:
        assert torch.equal(getattr(got, key), getattr(one, key)), key


def test_composite_chunks_of_a_long_ray(sdfr, oracle_mod, renderer_sd):
    """8c. N = 2050: the compositing kernel holds at most 2047 samples of a ray in LDS, so
    each ray takes two chunks (2047 + 3) with the transmittance and the accumulators
    carried in registers.  The maps against a float64 composite of the call's own fp32
    sdf / eikonal; the bound is the fp32 rounding of a front-to-back composite of N terms,
    (2 N + 4) 2^-24 of the largest map value (the s-th weight carries about s + 4 roundings
    of the running product, exp, sigmoid and the divisions; the sum N more)."""
    B, res, N = 1, 3, 2050
    ren = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True)
    cam, focal, near, far, lat, tr = _cameras(sdfr, res, B, 31)
    geo = _geo(ren, cam, focal, near, far, lat, tr)
    assert geo.sdf.shape == (B, res, res, N, 1) and geo.eikonal.abs().max() > 0
    g = dict(ext=cam.cpu().numpy(), focal=focal.cpu().numpy(), near=near.cpu().numpy(),
             far=far.cpu().numpy(), t_rand=tr.numpy())
    ray = _oracle_rays(oracle_mod, g, ren)
    tp = torch.from_numpy(_network_points(ray, g, True)).to(DEV)
    with torch.no_grad():
        sdf_q, _ = ren.query_gradient(tp, lat)
    assert torch.equal(geo.sdf.reshape(B, -1), sdf_q)
    ref = _maps64(geo.sdf[..., 0].cpu().numpy(), geo.eikonal.cpu().numpy(), ray,
                  float(ren.sigmoid_beta.detach()), False)
    bound = (2 * N + 4) * 2.0 ** -24
    for key in MAPS:
        got = _nhwc(getattr(geo, key)).astype(np.float64)
        err, scale = float(np.abs(got - ref[key]).max()), float(np.abs(ref[key]).max())
        _record[f"geometry:long_ray:{key}64"] = [err, scale]
        print(f"N {N} {key}: max err {err:.3e} at max |map| {scale:.3e} (bound {bound * scale:.3e})")
        assert err <= bound * scale, f"{key}: {err:.3e} > {bound * scale:.3e}"
    # the last sample's weight is not trivial here: the front of the ray absorbs part
    assert 0 < float(geo.mask.min()) and float(geo.mask.max()) < 1
    for key in ("depth", "eikonal"):
        got = _geo(ren, cam, focal, near, far, lat, tr, want=(key,))
        assert torch.equal(getattr(got, key), getattr(geo, key)), key


def test_geometry_deterministic(sdfr, golden_dir, renderer_sd):
    """9. Two calls give equal bits."""
    g = np.load(golden_dir / "render_face64.npz")
    ren = make_renderer(sdfr, renderer_sd, int(g["res"]), int(g["n_samples"]), return_sdf=True)
    cam, focal, near, far, lat, tr = _inputs(g)
    a = _geo(ren, cam, focal, near, far, lat, tr)
    b = _geo(ren, cam, focal, near, far, lat, tr)
    for key in ALL:
        assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert torch.isfinite(getattr(a, key)).all()


def test_generator_render_geometry_maps_styles_then_renders(sdfr):
    """10. Generator.render_geometry = forward's mapping network and truncation, then
    renderer.render_geometry, bit for bit."""
    opt = sdfr.vol_render_opt()
    opt.model.renderer_spatial_output_dim = 8
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    res = g.renderer.out_im_res
    z = torch.randn(2, 256, device=DEV)
    mean = [torch.randn(1, 256, device=DEV) * 0.1]
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, DEV, batch=2)
    tr = torch.rand(2, res, res)
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z], None, 0.7, mean, False)[0]
        assert g.renderer._query_fused_ok(ext, lat)
        want = g.renderer.render_geometry(ext, focal, near, far, lat, t_rand=tr, want=ALL)
        got = g.render_geometry([z], ext, focal, near, far, truncation=0.7,
                                truncation_latent=mean, t_rand=tr, want=ALL)
        same = g.render_geometry([lat.unsqueeze(1)], ext, focal, near, far,
                                 input_is_latent=True, t_rand=tr, want=ALL)
        unit = g.render_geometry([z], ext, focal, near, far, truncation=0.7,
                                 truncation_latent=mean, t_rand=tr, normalize=True,
                                 chunk_points=3 * res * g.renderer.N_samples)
        want_unit = g.renderer.render_geometry(ext, focal, near, far, lat, t_rand=tr,
                                               normalize=True)
    assert isinstance(got, sdfr.Geometry) and want.eikonal.abs().max() > 0
    for key in ALL:
        assert torch.equal(getattr(got, key), getattr(want, key)), key
        assert torch.equal(getattr(same, key), getattr(want, key)), key
    assert unit.sdf is None and unit.eikonal is None
    for key in MAPS:
        assert torch.equal(getattr(unit, key), getattr(want_unit, key)), key

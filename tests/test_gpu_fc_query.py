"""GPU: the fused FC field query and SDF gradient (sdfr_query_fc_forward, sdfr_query_fc_grad;
VolumeFeatureRenderer.query / query_gradient on an FCGenerator) against the reference's
fixture, the fused render, the float64 reference of tests/test_fc_query.py, the op-by-op
fp32 module path, and the mesh helpers and Generator calls on top."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden import weights as W
from tests.test_fc_query import (MAX_LEFT_OUT, POINT_MAX, alive_inputs, alive_renderer,
                                 module_grad, point_err, ref64)
from tests.test_gpu_fc import RTOL, make_fc
from tests.test_gpu_render import DEV, _inputs
from tests.test_gpu_siren_query import RATIO, _render_points

pytestmark = pytest.mark.gpu

GROUP = 32             # points per group with a per-face direction; per gradient pass

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


# ---------------------------------------------------------------------------- set-up
@pytest.fixture(scope="module")
def fc_sd(golden_dir):
    return W.det_state_dict(W.golden_entries(golden_dir, kind="fc"), "renderer.")


@pytest.fixture(scope="module")
def golden(sdfr, golden_dir, fc_sd):
    """Set (b): the golden FC weights (dead beyond layer 2, |grad| about 1e-8), the
    fixture's cameras and latents."""
    g = np.load(golden_dir / "render_fc_small.npz")
    ren = make_fc(sdfr, fc_sd, int(g["res"]), int(g["n_samples"]), return_sdf=True)
    return g, ren, _inputs(g)


@pytest.fixture(scope="module")
def alive(sdfr):
    """Set (a) on the GPU with its float64 reference, computed once."""
    ren = alive_renderer(sdfr)
    pts, lat = alive_inputs()
    ref = ref64(ren, pts, None, lat)
    return ren.to(DEV), pts.to(DEV), lat.to(DEV), ref


def _module_query(ren, tp, td, lat):
    """The op-by-op fp32 path on the GPU (the parent's query on an FC renderer)."""
    B, M = tp.shape[:2]
    d = td if td.dim() == 3 else td.unsqueeze(1).expand(B, M, 3)
    with torch.no_grad():
        raw = ren.network(torch.cat([tp, d], -1), styles=lat)
    return raw[..., 3].cpu().numpy(), torch.sigmoid(raw[..., :3]).cpu().numpy()


def _check(name, fused, module, ref):
    """The 3x mean-error rule on element-wise errors; every figure is printed and recorded
    before it is asserted."""
    ef = np.abs(np.asarray(fused, np.float64) - ref)
    em = np.abs(np.asarray(module, np.float64) - ref)
    _record[f"{name}:fused"] = [float(ef.max()), float(ef.mean())]
    _record[f"{name}:module"] = [float(em.max()), float(em.mean())]
    _record[f"{name}:scale"] = float(np.abs(ref).mean())
    print(f"{name}: fused max {ef.max():.3e} mean {ef.mean():.3e} | module max {em.max():.3e} "
          f"mean {em.mean():.3e} | mean |ref| {np.abs(ref).mean():.3e}")
    assert np.isfinite(np.asarray(fused)).all(), f"{name}: non-finite fused result"
    assert ef.mean() <= RATIO * em.mean(), \
        f"{name}: fused mean err {ef.mean():.3e} > {RATIO} x module {em.mean():.3e}"


def _check_grad(name, fused, module, ref):
    """The gradient on the reference's kept points: the 3x rule on the mean of the per-point
    errors (of max |grad|), and no kept point of the fused result above POINT_MAX."""
    keep = ref["keep"]
    left_out = 1.0 - float(keep.mean())
    ef, em = point_err(fused, ref["grad"])[keep], point_err(module, ref["grad"])[keep]
    gmax = float(np.linalg.norm(ref["grad"], axis=-1).max())
    _record[f"{name}:fused"] = [float(ef.max()), float(ef.mean())]
    _record[f"{name}:module"] = [float(em.max()), float(em.mean())]
    _record[f"{name}:max_grad"] = gmax
    _record[f"{name}:left_out"] = left_out
    print(f"{name}: of max |grad| = {gmax:.3e}: fused max {ef.max():.3e} mean {ef.mean():.3e} | "
          f"module max {em.max():.3e} mean {em.mean():.3e} | left out {left_out:.4f}")
    assert np.isfinite(np.asarray(fused)).all(), f"{name}: non-finite fused result"
    assert left_out <= MAX_LEFT_OUT
    assert ef.mean() <= RATIO * em.mean(), \
        f"{name}: fused mean err {ef.mean():.3e} > {RATIO} x module {em.mean():.3e}"
    assert ef.max() <= POINT_MAX, f"{name}: a kept point is {ef.max():.3e} of max |grad| away"


def _raw_query(sdfr, ren, pts, dirs, lat, prepacked=None):
    """sdfr_query_fc_forward on [B,R,N,3] / [B,R,3] with NaN-filled outputs."""
    B, R, N = pts.shape[:3]
    L = sdfr._lib.lib()
    sdf = torch.full((B, R, N), float("nan"), device=DEV)
    rgb = torch.full((B, R, N, 3), float("nan"), device=DEV)
    ws = torch.empty(L.sdfr_query_fc_workspace_bytes(B, R, N), dtype=torch.uint8, device=DEV)
    pts, dirs, lat = pts.contiguous(), dirs.contiguous(), lat.contiguous()
    w = ren._weight_struct(2)
    a = sdfr._lib.FcQueryArgs(
        B=B, R=R, N=N, points=sdfr._lib.ptr(pts), dirs=sdfr._lib.ptr(dirs),
        styles=sdfr._lib.ptr(lat), sdf=sdfr._lib.ptr(sdf), rgb=sdfr._lib.ptr(rgb),
        workspace=sdfr._lib.ptr(ws), workspace_bytes=ws.numel(),
        prepacked=sdfr._lib.ptr(prepacked))
    sdfr._lib.check(L.sdfr_query_fc_forward(ctypes.byref(w), ctypes.byref(a),
                                            sdfr._lib.stream_of(pts)), "query_fc")
    torch.cuda.synchronize()
    return sdf, rgb


def _raw_grad(sdfr, ren, pts, lat, prepacked=None):
    B, M = pts.shape[:2]
    L = sdfr._lib.lib()
    sdf = torch.full((B, M), float("nan"), device=DEV)
    grad = torch.full((B, M, 3), float("nan"), device=DEV)
    ws = torch.empty(L.sdfr_query_fc_grad_workspace_bytes(B, M), dtype=torch.uint8, device=DEV)
    pts, lat = pts.contiguous(), lat.contiguous()
    w = ren._weight_struct(2)
    a = sdfr._lib.FcGradArgs(
        B=B, M=M, points=sdfr._lib.ptr(pts), styles=sdfr._lib.ptr(lat),
        sdf=sdfr._lib.ptr(sdf), grad=sdfr._lib.ptr(grad), workspace=sdfr._lib.ptr(ws),
        workspace_bytes=ws.numel(), prepacked=sdfr._lib.ptr(prepacked))
    sdfr._lib.check(L.sdfr_query_fc_grad(ctypes.byref(w), ctypes.byref(a),
                                         sdfr._lib.stream_of(pts)), "query_fc_grad")
    torch.cuda.synchronize()
    return sdf, grad


# ---------------------------------------------------------------------------- 1
def test_fused_path_is_taken(alive, golden):
    """1. An FC renderer's point calls run fused on the GPU (the parent answers False and
    goes through self.network op by op)."""
    ren, pts, lat, _ = alive
    _, gren, inputs = golden
    with torch.no_grad():
        assert ren._net_kind() == 2 and ren._query_fused_ok(pts, lat)
        assert gren._query_fused_ok(inputs[0], inputs[4])
        with pytest.raises(ValueError, match="encode_only"):
            ren.query_gradient(pts, lat, encode_only=True)


# ---------------------------------------------------------------------------- 2
def test_query_at_render_samples_vs_reference_and_render(golden):
    """2. The query at the render's own sample points (B = 2, two latents): against the
    reference's per-sample SDF under the bound the fused render meets on the same fixture,
    and equal to the fused render's return_sdf bit for bit."""
    g, ren, (cam, focal, near, far, lat, tr) = golden
    with torch.no_grad():
        out = ren(cam, focal, near, far, styles=lat, t_rand=tr)
    pts, dirs = _render_points(ren, cam, focal, near, far, tr)
    with torch.no_grad():
        sdf, rgb = ren._fused_query(pts, dirs, lat)
    torch.cuda.synchronize()
    B, res, N = 2, int(g["res"]), int(g["n_samples"])
    assert sdf.shape == (B, res * res, N) and rgb.shape == (B, res * res, N, 3)
    ref = np.asarray(g["sdf"], np.float64)
    err = float(np.abs(sdf.cpu().double().numpy().reshape(ref.shape) - ref).max())
    err /= float(np.abs(ref).max())
    _record["fc_query_render_fc_small:sdf"] = err
    print(f"query vs render_fc_small sdf: rel max {err:.3e} (bound {RTOL['sdf']:.1e})")
    assert err <= RTOL["sdf"]
    assert not torch.equal(sdf[0], sdf[1])
    assert torch.equal(sdf.reshape(out[2].shape), out[2])
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0


# ---------------------------------------------------------------------------- 3
@pytest.mark.parametrize("B,R,N", [(2, 17, 3), (1, 1, 1), (2, 16, 33)])
def test_raw_query_writes_every_element(sdfr, alive, B, R, N):
    """3. Ragged group and point counts with NaN-filled outputs: every element written, the
    caller's prepacked buffer and packing inside the workspace give equal bits, and the same
    points in groups of N = 1 give the same SDF (no dependence on the grouping)."""
    ren, pts, lat, _ = alive
    p = pts[:B, :R * N].reshape(B, R, N, 3).contiguous()
    d = F.normalize(torch.randn(B, R, 3, generator=torch.Generator().manual_seed(R)), dim=-1)
    d = d.to(DEV)
    sdf, rgb = _raw_query(sdfr, ren, p, d, lat[:B])
    assert torch.isfinite(sdf).all() and torch.isfinite(rgb).all()
    sdf_p, rgb_p = _raw_query(sdfr, ren, p, d, lat[:B], prepacked=ren._prepacked(2, p))
    assert torch.equal(sdf, sdf_p) and torch.equal(rgb, rgb_p)
    d1 = d.unsqueeze(2).expand(B, R, N, 3).reshape(B, R * N, 3)
    sdf_1, rgb_1 = _raw_query(sdfr, ren, p.reshape(B, R * N, 1, 3), d1, lat[:B])
    assert torch.equal(sdf_1.reshape(B, R, N), sdf)
    assert torch.equal(rgb_1.reshape(B, R, N, 3), rgb)


def test_group_size_does_not_change_the_sdf(alive):
    """3. Groups of N = 1 (a direction per point) and N = 32 (a direction per face) give
    equal SDF at the same points, through the Python call's padding and trimming."""
    ren, pts, lat, _ = alive
    p = pts[:, :3 * GROUP + 5].contiguous()
    d = F.normalize(torch.randn(2, p.shape[1], 3, device=DEV), dim=-1)
    with torch.no_grad():
        sdf_pp, rgb_pp = ren.query(p, lat, viewdirs=d)
        sdf_pf, rgb_pf = ren.query(p, lat, viewdirs=d[:, 0])
        only_sdf, none = ren.query(p, lat, return_rgb=False)
    assert sdf_pp.shape == (2, p.shape[1]) and rgb_pf.shape == (2, p.shape[1], 3)
    assert none is None
    assert torch.equal(sdf_pp, sdf_pf) and torch.equal(only_sdf, sdf_pp)
    assert torch.equal(rgb_pp[:, 0], rgb_pf[:, 0])          # point 0 has the face's direction


# ---------------------------------------------------------------------------- 4
def test_query_generic_points_colour_and_range(alive):
    """4. 2 x 41 points in [-2.2, 2.2]^3, one the origin: sdf and rgb with a direction per
    point (N = 1 groups) and per face (N = 32 groups) against the float64 reference,
    measured against the fp32 module path."""
    ren, _, lat, _ = alive
    rng = np.random.default_rng(11)
    pts = rng.uniform(-2.2, 2.2, (2, 41, 3)).astype(np.float32)
    pts[:, -1] = 0.0
    dirs = rng.normal(size=(2, 41, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    tp, td = torch.from_numpy(pts).to(DEV), torch.from_numpy(dirs).to(DEV)
    ref_pp, ref_pf = ref64(ren, pts, dirs, lat), ref64(ren, pts, dirs[:, 0], lat)
    with torch.no_grad():
        sdf_pp, rgb_pp = ren.query(tp, lat, viewdirs=td)
        sdf_pf, rgb_pf = ren.query(tp, lat, viewdirs=td[:, 0])
    assert torch.equal(sdf_pp, sdf_pf)
    m_sdf, m_rgb = _module_query(ren, tp, td, lat)
    _check("fc_query_points:sdf", sdf_pp.cpu().numpy(), m_sdf, ref_pp["sdf"])
    _check("fc_query_points:rgb", rgb_pp.cpu().numpy(), m_rgb, ref_pp["rgb"])
    _, m_rgb = _module_query(ren, tp, td[:, 0], lat)
    _check("fc_query_points:rgb_face", rgb_pf.cpu().numpy(), m_rgb, ref_pf["rgb"])


# ---------------------------------------------------------------------------- 5
def test_gradient_alive_weights(alive):
    """5. Set (a), 2 x 4096 points, the reference's kept points: the 3x mean rule, no kept
    point above 1e-3 of max |grad| (the maximum is recorded), and the call's sdf equal to
    the query's bit for bit."""
    ren, pts, lat, ref = alive
    with torch.no_grad():
        sdf, grad = ren.query_gradient(pts, lat)
        q_sdf, _ = ren.query(pts, lat, return_rgb=False)
    assert sdf.shape == (2, 4096) and grad.shape == (2, 4096, 3)
    m_sdf, m_grad = module_grad(ren, pts, lat)
    _check_grad("fc_grad_alive", grad.cpu().numpy(), m_grad, ref)
    _check("fc_grad_alive:sdf", sdf.cpu().numpy(), m_sdf, ref["sdf"])
    d = (sdf - q_sdf).abs()
    _record["fc_grad_alive:sdf_vs_query"] = [float(d.max()), float(d.mean())]
    assert torch.equal(sdf, q_sdf)


# ---------------------------------------------------------------------------- 6
def test_gradient_golden_weights(golden):
    """6. Set (b): gradients of about 1e-8 -- the tangent columns shrink by orders of
    magnitude per layer and live on their power-of-two exponents.  Finite, and the 3x
    rule on the reference's kept points."""
    _, ren, inputs = golden
    lat = inputs[4]
    pts = (torch.rand(2, 1024, 3, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    ref = ref64(ren, pts, None, lat)
    with torch.no_grad():
        sdf, grad = ren.query_gradient(pts, lat)
        q_sdf, _ = ren.query(pts, lat, return_rgb=False)
    assert torch.isfinite(grad).all() and torch.isfinite(sdf).all()
    assert torch.equal(sdf, q_sdf)
    # (the SDF of these weights is one constant, sigma_linear's bias plus 1e-8: its error is
    # which fp32 neighbour of the constant a path lands on, and is not compared here; the
    # call's sdf is the query's, which test 2 holds to the fixture)
    _, m_grad = module_grad(ren, pts, lat)
    _check_grad("fc_grad_golden", grad.cpu().numpy(), m_grad, ref)


# ---------------------------------------------------------------------------- 7
def test_gradient_passes_and_chunking(sdfr, alive):
    """7. B = 2, M = 32809: the launch caps a face's workgroups at 1024 / B = 512, and 1026
    passes of 32 points give two of them three passes, the last one partial (the weight ring
    running ahead across passes, the next pass's points loaded under the last layer).
    Fully written, and bit-equal to calls of M = 1 and M = 41 and to a call on each slice
    that starts at a multiple of 32 points; chunk_points / chunk_groups change no bit."""
    ren, pts, lat, _ = alive
    M = 32 * 1025 + 9
    big = (torch.rand(2, M, 3, generator=torch.Generator().manual_seed(23)) * 4.2 - 2.1).to(DEV)
    sdf, grad = _raw_grad(sdfr, ren, big, lat)
    assert torch.isfinite(sdf).all() and torch.isfinite(grad).all()
    for i0, i1 in ((0, 1), (0, 41), (32 * 300, 32 * 300 + 41), (32 * 512, 32 * 513),
                   (32 * 1024, M)):
        s, g = _raw_grad(sdfr, ren, big[:, i0:i1], lat)
        assert torch.isfinite(s).all() and torch.isfinite(g).all()
        assert torch.equal(s, sdf[:, i0:i1]) and torch.equal(g, grad[:, i0:i1]), (i0, i1)
    s_p, g_p = _raw_grad(sdfr, ren, big, lat, prepacked=ren._prepacked(2, big))
    assert torch.equal(s_p, sdf) and torch.equal(g_p, grad)
    p = big[:, :32 * 40 + 5].contiguous()
    d = F.normalize(torch.randn(2, 3, device=DEV), dim=-1)
    with torch.no_grad():
        gs1, g1 = ren.query_gradient(p, lat)
        gs3, g3 = ren.query_gradient(p, lat, chunk_points=64)
        sdf1, rgb1 = ren.query(p, lat, viewdirs=d)
        sdf3, rgb3 = ren.query(p, lat, viewdirs=d, chunk_groups=16)
    assert torch.equal(gs1, sdf[:, :p.shape[1]]) and torch.equal(g1, grad[:, :p.shape[1]])
    assert torch.equal(gs1, gs3) and torch.equal(g1, g3)
    assert torch.equal(sdf1, sdf3) and torch.equal(rgb1, rgb3) and torch.equal(sdf1, gs1)


# ---------------------------------------------------------------------------- 8
def test_generator_calls_equal_renderer_calls(sdfr):
    """8. Generator.query_field / query_field_gradient on an FC generator = forward's
    mapping network and truncation, then the renderer-level calls, bit for bit."""
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    assert g.renderer._net_kind() == 2
    z = torch.randn(2, 256, device=DEV)
    mean = [torch.randn(1, 256, device=DEV) * 0.1]
    pts = torch.rand(2, 40, 3, device=DEV) - 0.5
    d = torch.tensor([[0.0, 0.0, -1.0]] * 2, device=DEV)
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z], None, 0.7, mean, False)[0]
        assert g.renderer._query_fused_ok(pts, lat)
        want = g.renderer.query(pts, lat, viewdirs=d)
        got = g.query_field(pts, [z], viewdirs=d, truncation=0.7, truncation_latent=mean)
        want_g = g.renderer.query_gradient(pts, lat)
        got_g = g.query_field_gradient(pts, [z], truncation=0.7, truncation_latent=mean)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got_g[0], want_g[0]) and torch.equal(got_g[1], want_g[1])
    assert torch.isfinite(want_g[1]).all()


def test_mesh_helpers_run_fused(sdfr, alive):
    """8. sdf_cube at res 24 equals renderer.query on cube_points; marching cubes ->
    color_mesh, normal_mesh, eikonal_residual on the fused path.  The seeded field is
    negative on the whole cube, so sigma_linear's bias is moved to put the cube's median
    SDF at zero (the choice looks at the SDF only).  Normals against the module path on the
    vertices the float64 reference keeps: both paths are within POINT_MAX of max |grad| of
    the reference there, so by first-order propagation through g / |g| they are within
    2 POINT_MAX max |grad| / min |grad| of each other."""
    ren0, _, lat, _ = alive
    ren = copy.deepcopy(ren0)
    lat1 = lat[:1]
    res = 24
    cp = sdfr.cube_points(res, DEV).reshape(1, -1, 3)
    with torch.no_grad():
        assert ren._query_fused_ok(cp, lat1)
        ren.network.sigma_linear.bias -= ren.query(cp, lat1, return_rgb=False)[0].median()
        cube = sdfr.sdf_cube(ren, lat1, res=res)
        q_sdf, _ = ren.query(cp, lat1, return_rgb=False)
    assert cube.shape == (1, res, res, res, 1)
    assert torch.equal(cube.reshape(1, -1), q_sdf)
    below = float((cube < 0).float().mean())
    assert 0.2 < below < 0.8, below
    mesh = sdfr.extract_mesh_with_marching_cubes(cube)
    V = len(mesh.vertices)
    assert V > 0
    col = sdfr.color_mesh(mesh, ren, lat1)
    assert col.shape == (V, 3) and col.min() >= 0.0 and col.max() <= 1.0
    n = sdfr.normal_mesh(mesh, ren, lat1)
    assert n.shape == (V, 3)
    v = sdfr.world_to_network(torch.from_numpy(mesh.vertices).to(DEV)).unsqueeze(0)
    ref = ref64(ren, v, None, lat1)
    keep = ref["keep"][0]
    assert keep.mean() >= 0.5                               # (the comparison is not vacuous)
    module = module_grad(ren, v, lat1)[1][0].astype(np.float64)
    norm = np.linalg.norm(module, axis=-1)
    gmin, gmax = float(norm[keep].min()), float(np.linalg.norm(ref["grad"], axis=-1).max())
    assert gmin > 0
    np.testing.assert_allclose(np.linalg.norm(n[keep], axis=-1), 1.0, rtol=0, atol=1e-6)
    m_unit = module / norm[:, None]
    bound = 2 * POINT_MAX * gmax / gmin
    err = float(np.abs(n - m_unit)[keep].max())
    _record["fc_mesh:normal_vs_module"] = [err, bound, gmin, gmax]
    print(f"normals vs module path on {int(keep.sum())} of {V} vertices: max {err:.3e} "
          f"(bound {bound:.3e}, |grad| min {gmin:.3e} max {gmax:.3e})")
    assert err <= bound
    res_e = sdfr.eikonal_residual(ren, lat1, v)
    assert res_e.shape == (1, V) and torch.isfinite(res_e).all()


def test_surface_and_geometry_renders_stay_op_by_op(golden):
    """8. render_surface and render_geometry of an FC renderer on the GPU are still
    _module_surface and _module_geometry: the fused point calls do not reroute them."""
    _, ren, (cam, focal, near, far, lat, tr) = golden
    want_s = ("hit", "sample", "depth", "xyz", "normal", "rgb", "residual", "sdf")
    want_g = ("normal", "depth", "xyz", "mask", "sdf", "eikonal")
    with torch.no_grad():
        assert ren._query_fused_ok(cam, lat)
        surf = ren.render_surface(cam, focal, near, far, lat, t_rand=tr, refine_steps=2,
                                  want=want_s)
        mod_s = ren._module_surface(cam, focal, near, far, lat, tr, 2, want_s)
        geo = ren.render_geometry(cam, focal, near, far, lat, t_rand=tr, want=want_g)
        mod_g = ren._module_geometry(cam, focal, near, far, lat, tr, want_g)
    for k in want_s:
        assert torch.equal(getattr(surf, k), mod_s[k]), k
    for k in want_g:
        assert torch.equal(getattr(geo, k), mod_g[k]), k


# ---------------------------------------------------------------------------- 9
def test_argument_checks_on_device_tensors(sdfr, alive):
    """9. SDFR_EINVAL for a null sdf, a short workspace and zero sizes, SDFR_EUNSUPPORTED
    for depth 7 -- with real device pointers, and nothing is written."""
    ren, pts, lat, _ = alive
    L, lib = sdfr._lib.lib(), sdfr._lib
    p = pts[:1, :64].reshape(1, 2, 32, 3).contiguous()
    d = torch.zeros(1, 2, 3, device=DEV)
    l1 = lat[:1].contiguous()
    sdf = torch.full((1, 2, 32), float("nan"), device=DEV)
    grad = torch.full((1, 64, 3), float("nan"), device=DEV)
    ws = torch.empty(L.sdfr_query_fc_workspace_bytes(1, 2, 32), dtype=torch.uint8, device=DEV)
    assert ws.numel() == L.sdfr_query_fc_grad_workspace_bytes(1, 64)

    def q(w=None, **kw):
        f = dict(B=1, R=2, N=32, points=lib.ptr(p), dirs=lib.ptr(d), styles=lib.ptr(l1),
                 sdf=lib.ptr(sdf), rgb=None, workspace=lib.ptr(ws), workspace_bytes=ws.numel(),
                 prepacked=None)
        f.update(kw)
        return L.sdfr_query_fc_forward(ctypes.byref(w or ren._weight_struct(2)),
                                       ctypes.byref(lib.FcQueryArgs(**f)), lib.stream_of(p))

    def g(w=None, **kw):
        f = dict(B=1, M=64, points=lib.ptr(p), styles=lib.ptr(l1), sdf=None,
                 grad=lib.ptr(grad), workspace=lib.ptr(ws), workspace_bytes=ws.numel(),
                 prepacked=None)
        f.update(kw)
        return L.sdfr_query_fc_grad(ctypes.byref(w or ren._weight_struct(2)),
                                    ctypes.byref(lib.FcGradArgs(**f)), lib.stream_of(p))

    w7 = ren._weight_struct(2)
    w7.depth = 7
    assert q(sdf=None) == lib.SDFR_EINVAL and g(grad=None) == lib.SDFR_EINVAL
    assert q(workspace_bytes=ws.numel() - 1) == lib.SDFR_EINVAL
    assert g(workspace_bytes=ws.numel() - 1) == lib.SDFR_EINVAL
    for zero in ("B", "R", "N"):
        assert q(**{zero: 0}) == lib.SDFR_EINVAL
    for zero in ("B", "M"):
        assert g(**{zero: 0}) == lib.SDFR_EINVAL
    assert q(w=w7) == lib.SDFR_EUNSUPPORTED and g(w=w7) == lib.SDFR_EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(sdf).all() and torch.isnan(grad).all()
    assert q() == lib.SDFR_OK and g() == lib.SDFR_OK
    torch.cuda.synchronize()
    assert torch.isfinite(sdf).all() and torch.isfinite(grad).all()

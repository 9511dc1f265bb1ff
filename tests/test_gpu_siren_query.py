"""GPU: the fused SIREN field query and SDF gradient (sdfr_query_siren_forward,
sdfr_query_siren_grad; VolumeFeatureRenderer.query / query_gradient on a SirenGenerator)
against the reference's fixtures, the fused render, a float64 run of the same module, the
op-by-op fp32 module path, and the mesh helpers and Generator calls on top."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden import weights as W
from tests.test_gpu_render import DEV, _cmp, _inputs, make_siren
from tests.test_gpu_stage1 import _stage1_generator

pytestmark = pytest.mark.gpu

P_HALF = 8             # groups of a wave pair (query) / points of a wave pass (gradient)
TILE = 16              # groups per tile (query)
GROUP = 32             # points per group with a per-face direction; per gradient pass
PASS = 4               # kPSamples: points of a group per pass of the query kernel
# The project's margin for split-fp16 against fp32 (tests/test_gpu_query_gradient.py): the
# fused mean error may be at most 3x the op-by-op fp32 module path's, both against the same
# float64 evaluation.
RATIO = 3.0
# max |grad - ref64| tripwire: 3x the value measured on MI355X over the generic points
# (mean |grad| 0.80) and their x8 set (0.71), profiles/siren_gradient_parity.json keys
# "siren_grad_points:fused" and "siren_grad_points_x8:fused" (first entry: max; the
# op-by-op path measures 3.67e-5 and 2.03e-4 there, ":module").  The inputs are seeded and
# the kernel deterministic, so the bound is a regression tripwire, not a noise allowance.
MEASURED_MAX = {"siren_grad_points": 6.117e-05, "siren_grad_points_x8": 4.612e-04}
# The project's relative bounds for the eikonal term and the SDF of eikonal_siren.npz
# (tests/test_geometry.py:176, tests/test_gpu_stage1.py): of the largest magnitude.
REL_EIKONAL, REL_SDF = 1e-4, 2e-5

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
def siren_sd(golden_dir):
    return W.det_state_dict(W.golden_entries(golden_dir, siren=True), "renderer.")


@pytest.fixture(scope="module")
def ren(sdfr, siren_sd):
    return make_siren(sdfr, siren_sd, 8, 24, return_sdf=True)


@pytest.fixture(scope="module")
def ren64(ren):
    """The same module in float64 on the CPU: the reference of the accuracy tests."""
    return copy.deepcopy(ren).cpu().double()


@pytest.fixture(scope="module")
def lat(golden_dir):
    return torch.from_numpy(np.load(golden_dir / "render_siren_small.npz")["latent"]).to(DEV)


def _ref64(ren64, pts, dirs, lat):
    """(sdf [B,M], rgb [B,M,3] in [0,1], grad [B,M,3]) of the float64 module."""
    p = torch.as_tensor(pts).double().cpu().clone().requires_grad_(True)
    B, M = p.shape[:2]
    d = torch.as_tensor(dirs).double().cpu()
    d = d if d.dim() == 3 else d.unsqueeze(1).expand(B, M, 3)
    raw = ren64.network(torch.cat([p, d], -1), styles=torch.as_tensor(lat).double().cpu())
    grad, = torch.autograd.grad(raw[..., 3].sum(), p)
    return (raw[..., 3].detach().numpy(), torch.sigmoid(raw[..., :3]).detach().numpy(),
            grad.numpy())


def _module_query(ren, tp, td, lat):
    """The op-by-op fp32 path on the GPU (the parent's query on a SIREN renderer)."""
    B, M = tp.shape[:2]
    d = td if td.dim() == 3 else td.unsqueeze(1).expand(B, M, 3)
    with torch.no_grad():
        raw = ren.network(torch.cat([tp, d], -1), styles=lat)
    return raw[..., 3].cpu().numpy(), torch.sigmoid(raw[..., :3]).cpu().numpy()


def _module_grad(ren, tp, lat):
    """The op-by-op fp32 path: autograd through renderer.network on the GPU."""
    p = tp.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        raw = ren.network(torch.cat([p, torch.zeros_like(p)], -1), styles=lat.detach())
        g, = torch.autograd.grad(raw[..., 3].sum(), p)
    return g.cpu().numpy()


def _check(name, fused, module, ref, max_key=None):
    """The 3x mean-error rule (and, with max_key, the max-error tripwire); every figure is
    printed and recorded before it is asserted."""
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
    if max_key is not None:
        bound = 3 * MEASURED_MAX[max_key]
        assert ef.max() <= bound, f"{name}: fused max err {ef.max():.3e} > {bound:.3e}"


def _render_points(ren, cam, focal, near, far, t_rand):
    """The render's sample points as the reference forms them, in fp32 on the CPU
    (camera_rays + sample_points): network coordinates [B,HW,N,3], directions [B,HW,3] as
    the network sees them."""
    r = copy.deepcopy(ren).cpu()
    c = lambda t: t.detach().cpu()  # noqa: E731
    with torch.no_grad():
        ro, rd, vd, nr, fr = r.camera_rays(c(focal), c(cam), c(near), c(far))
        _, _, npts = r.sample_points(ro, rd, nr, fr, t_rand, r._stratify())
    B, H, Wd, N = npts.shape[:4]
    return (npts.reshape(B, H * Wd, N, 3).contiguous().to(DEV),
            vd.reshape(B, H * Wd, 3).float().contiguous().to(DEV))


def _fixture_case(sdfr, golden_dir, siren_sd, name, flags):
    g = np.load(golden_dir / f"{name}.npz")
    ren = make_siren(sdfr, siren_sd, int(g["res"]), int(g["n_samples"]), **flags)
    cam, focal, near, far, lat, tr = _inputs(g)
    with torch.no_grad():
        out = ren(cam, focal, near, far, styles=lat, t_rand=tr)
    pts, dirs = _render_points(ren, cam, focal, near, far, tr)
    with torch.no_grad():
        assert ren._query_fused_ok(pts, lat)
        sdf, rgb = ren._fused_query(pts, dirs, lat)
    torch.cuda.synchronize()
    return g, out, sdf, rgb


SDF_CASES = [
    ("render_siren_face32", dict(return_sdf=True, return_xyz=True)),
    ("render_siren_mesh_opts", dict(static_viewdirs=True, force_background=True, perturb=0,
                                    return_sdf=True, return_xyz=True)),
]


# ---------------------------------------------------------------------------- 4, 5
@pytest.mark.parametrize("name,flags", SDF_CASES)
def test_query_at_render_samples_vs_reference_and_render(sdfr, golden_dir, siren_sd, name, flags):
    """4. The query at the render's own sample points against the reference's per-sample
    SDF, under the bound the fused render meets on the same fixture.  5. And equal to the
    fused render's return_sdf bit for bit: same packed weights, FiLM vectors, k-step order."""
    g, out, sdf, rgb = _fixture_case(sdfr, golden_dir, siren_sd, name, flags)
    B, res, N = sdf.shape[0], int(g["res"]), int(g["n_samples"])
    assert sdf.shape == (B, res * res, N) and rgb.shape == (B, res * res, N, 3)
    _cmp(f"siren_query_{name}", "sdf", sdf.cpu().numpy(), g["sdf"])
    assert torch.equal(sdf.reshape(out[2].shape), out[2])
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0


def test_query_equals_render_two_faces(sdfr, golden_dir, siren_sd):
    """5. B = 2 with two different latents: a FiLM block of the wrong face shows here."""
    g, out, sdf, _ = _fixture_case(sdfr, golden_dir, siren_sd, "render_siren_small",
                                   dict(return_sdf=True))
    assert sdf.shape[0] == 2 and not torch.equal(sdf[0], sdf[1])
    assert torch.equal(sdf.reshape(out[2].shape), out[2])


# ---------------------------------------------------------------------------- 6, 8
def _generic_points(scale=1.0):
    """2 x 41 seeded points in [-2.2, 2.2]^3 times `scale`, the last one the origin, and a
    unit direction per point."""
    rng = np.random.default_rng(11)
    pts = (rng.uniform(-2.2, 2.2, (2, 41, 3)) * scale).astype(np.float32)
    pts[:, -1] = 0.0
    dirs = rng.normal(size=(2, 41, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    return pts, dirs


@pytest.fixture(scope="module", params=[1.0, 8.0], ids=["x1", "x8"])
def generic(request, ren, ren64, lat):
    pts, dirs = _generic_points(request.param)
    assert np.abs(pts).max() <= 64                          # the documented range
    tp, td = torch.from_numpy(pts).to(DEV), torch.from_numpy(dirs).to(DEV)
    tag = "" if request.param == 1.0 else "_x8"
    return dict(tag=tag, pts=pts, dirs=dirs, tp=tp, td=td,
                ref_pp=_ref64(ren64, pts, dirs, lat), ref_pf=_ref64(ren64, pts, dirs[:, 0], lat))


def test_query_generic_points_colour_and_range(ren, generic, lat):
    """6. sdf and rgb with a direction per point (N = 1 groups) and per face (N = 32
    groups) against float64, measured against the fp32 module path; the x8 set and the
    origin cover the coordinate range."""
    g = generic
    with torch.no_grad():
        assert ren._query_fused_ok(g["tp"], lat)
        sdf_pp, rgb_pp = ren.query(g["tp"], lat, viewdirs=g["td"])
        sdf_pf, rgb_pf = ren.query(g["tp"], lat, viewdirs=g["td"][:, 0])
        only_sdf, none = ren.query(g["tp"], lat, return_rgb=False)
    assert sdf_pp.shape == (2, 41) and rgb_pf.shape == (2, 41, 3) and none is None
    assert torch.equal(sdf_pp, sdf_pf) and torch.equal(only_sdf, sdf_pp)
    m_sdf, m_rgb = _module_query(ren, g["tp"], g["td"], lat)
    _check(f"siren_query_points{g['tag']}:sdf", sdf_pp.cpu().numpy(), m_sdf, g["ref_pp"][0])
    _check(f"siren_query_points{g['tag']}:rgb", rgb_pp.cpu().numpy(), m_rgb, g["ref_pp"][1])
    m_sdf, m_rgb = _module_query(ren, g["tp"], g["td"][:, 0], lat)
    _check(f"siren_query_points{g['tag']}:rgb_face", rgb_pf.cpu().numpy(), m_rgb, g["ref_pf"][1])


def test_gradient_generic_points(ren, generic, lat):
    """8. grad against float64 autograd of the module and the fp32 module path (3x mean
    rule, max tripwire); the gradient call's sdf (field_r_kernel's loop: not the query's
    bits) under the same rule, its distance to the query's recorded."""
    g = generic
    with torch.no_grad():
        sdf, grad = ren.query_gradient(g["tp"], lat)
        q_sdf, _ = ren.query(g["tp"], lat, return_rgb=False)
    assert sdf.shape == (2, 41) and grad.shape == (2, 41, 3)
    name = f"siren_grad_points{g['tag']}"
    d = (sdf - q_sdf).abs()
    _record[f"{name}:sdf_vs_query"] = [float(d.max()), float(d.mean())]
    print(f"{name}: |grad-call sdf - query sdf| max {float(d.max()):.3e}")
    m_sdf, _ = _module_query(ren, g["tp"], g["td"], lat)
    _check(f"{name}:sdf", sdf.cpu().numpy(), m_sdf, g["ref_pp"][0])
    _check(name, grad.cpu().numpy(), _module_grad(ren, g["tp"], lat), g["ref_pp"][2],
           max_key=name)


# ---------------------------------------------------------------------------- 7
def _raw_query(sdfr, ren, pts, dirs, lat):
    """sdfr_query_siren_forward on [B,R,N,3] / [B,R,3] with NaN-filled outputs."""
    B, R, N = pts.shape[:3]
    L = sdfr._lib.lib()
    sdf = torch.full((B, R, N), float("nan"), device=DEV)
    rgb = torch.full((B, R, N, 3), float("nan"), device=DEV)
    ws = torch.empty(L.sdfr_query_siren_workspace_bytes(B, R, N), dtype=torch.uint8, device=DEV)
    pts, dirs, lat = pts.contiguous(), dirs.contiguous(), lat.contiguous()
    w = ren._weight_struct(1)
    a = sdfr._lib.SirenQueryArgs(
        B=B, R=R, N=N, points=sdfr._lib.ptr(pts), dirs=sdfr._lib.ptr(dirs),
        styles=sdfr._lib.ptr(lat), sdf=sdfr._lib.ptr(sdf), rgb=sdfr._lib.ptr(rgb),
        workspace=sdfr._lib.ptr(ws), workspace_bytes=ws.numel(), prepacked=None)
    sdfr._lib.check(L.sdfr_query_siren_forward(ctypes.byref(w), ctypes.byref(a),
                                               sdfr._lib.stream_of(pts)), "query_siren")
    torch.cuda.synchronize()
    return sdf, rgb


def _raw_grad(sdfr, ren, pts, lat):
    B, M = pts.shape[:2]
    L = sdfr._lib.lib()
    sdf = torch.full((B, M), float("nan"), device=DEV)
    grad = torch.full((B, M, 3), float("nan"), device=DEV)
    ws = torch.empty(L.sdfr_query_siren_grad_workspace_bytes(B, M), dtype=torch.uint8,
                     device=DEV)
    pts, lat = pts.contiguous(), lat.contiguous()
    w = ren._weight_struct(1)
    a = sdfr._lib.SirenGradArgs(
        B=B, M=M, points=sdfr._lib.ptr(pts), styles=sdfr._lib.ptr(lat),
        sdf=sdfr._lib.ptr(sdf), grad=sdfr._lib.ptr(grad), workspace=sdfr._lib.ptr(ws),
        workspace_bytes=ws.numel(), prepacked=None)
    sdfr._lib.check(L.sdfr_query_siren_grad(ctypes.byref(w), ctypes.byref(a),
                                            sdfr._lib.stream_of(pts)), "query_siren_grad")
    torch.cuda.synchronize()
    return sdf, grad


@pytest.fixture(scope="module")
def ragged(sdfr, ren, lat):
    """One larger call of each kind: 37 groups x 32 points per face, computed once."""
    rng = np.random.default_rng(5)
    pts = torch.from_numpy(rng.uniform(-2.1, 2.1, (2, 37, 32, 3)).astype(np.float32)).to(DEV)
    dirs = F.normalize(torch.from_numpy(rng.normal(size=(2, 37, 3)).astype(np.float32)), dim=-1)
    dirs = dirs.to(DEV)
    sdf, rgb = _raw_query(sdfr, ren, pts, dirs, lat)
    g_sdf, grad = _raw_grad(sdfr, ren, pts.reshape(2, -1, 3), lat)
    for t in (sdf, rgb, g_sdf, grad):
        assert torch.isfinite(t).all()
    return dict(pts=pts, dirs=dirs, sdf=sdf, rgb=rgb, g_sdf=g_sdf, grad=grad)


@pytest.mark.parametrize("R,N", [(1, 32), (P_HALF - 1, 3), (P_HALF + 1, 5), (TILE - 1, 1),
                                 (TILE + 1, PASS), (21, 1), (21, 3), (21, 5), (21, 32),
                                 (2 * TILE + 5, PASS + 1)])
def test_query_ragged_groups(sdfr, ren, ragged, lat, R, N):
    """7. R around the wave pair's 8 groups, the 16-group tile and the 32-group workgroup,
    N around the kPSamples = 4 pass: every output written (NaN pre-fill), and bit-equal to
    the same points inside the larger call -- no dependence on neighbours or padding."""
    r = ragged
    sdf, rgb = _raw_query(sdfr, ren, r["pts"][:, :R, :N], r["dirs"][:, :R], lat)
    assert torch.isfinite(sdf).all() and torch.isfinite(rgb).all()
    assert torch.equal(sdf, r["sdf"][:, :R, :N]) and torch.equal(rgb, r["rgb"][:, :R, :N])


@pytest.mark.parametrize("M", [1, P_HALF - 1, P_HALF + 1, GROUP - 1, GROUP + 1, 3 * GROUP + 5])
def test_query_and_gradient_ragged_points(sdfr, ren, ragged, lat, M):
    """7. M around the 8-point half, the 32-point group / pass and several of them, through
    the Python calls (padding and trimming) and the raw gradient call: fully written,
    bit-equal to the same points inside the larger call."""
    r = ragged
    flat = r["pts"].reshape(2, -1, 3)[:, :M].contiguous()
    g_sdf, grad = _raw_grad(sdfr, ren, flat, lat)
    assert torch.isfinite(g_sdf).all() and torch.isfinite(grad).all()
    assert torch.equal(g_sdf, r["g_sdf"][:, :M]) and torch.equal(grad, r["grad"][:, :M])
    with torch.no_grad():
        sdf, rgb = ren.query(flat, lat, viewdirs=r["dirs"][:, 0])
        s2, g2 = ren.query_gradient(flat, lat)
        sdf1, rgb1 = ren.query(flat, lat, viewdirs=r["dirs"][:, :1].expand(2, M, 3))
    assert sdf.shape == (2, M) and rgb.shape == (2, M, 3)
    assert torch.equal(s2, g_sdf) and torch.equal(g2, grad)
    assert torch.equal(sdf, r["sdf"].reshape(2, -1)[:, :M])
    # the colour depends on the direction: group 0's direction holds for the first 32 only
    k = min(M, GROUP)
    assert torch.equal(rgb[:, :k], r["rgb"].reshape(2, -1, 3)[:, :k])
    assert torch.equal(sdf1, sdf) and torch.equal(rgb1, rgb)     # N = 1 groups


# ---------------------------------------------------------------------------- 9
def test_gradient_vs_reference_eikonal_term(sdfr, golden_dir):
    """9. The reference's own eikonal term (autograd through its SIREN, eikonal_siren.npz):
    grad x 2 / (far - near) at the render's sample points, and the SDF, under the project's
    relative bounds for exactly these tensors; the module path's error beside it."""
    g = np.load(golden_dir / "eikonal_siren.npz")
    gen = _stage1_generator(sdfr, golden_dir, g, "siren").eval()
    t = lambda k: torch.from_numpy(g[k]).to(DEV)  # noqa: E731
    ren = gen.renderer
    with torch.no_grad():
        lat = gen.styles_and_noise_forward([t("z")])[0]
        pts, _ = _render_points(ren, t("ext"), t("focal"), t("near"), t("far"),
                                torch.from_numpy(g["t_rand"]))
        B, R, N = pts.shape[:3]
        flat = pts.reshape(B, R * N, 3)
        assert ren._query_fused_ok(flat, lat)
        sdf, grad = ren.query_gradient(flat, lat)
        q_sdf, _ = ren.query(flat, lat, return_rgb=False)
        ren.use_fused = False
        m_sdf, m_grad = ren.query_gradient(flat, lat)
        ren.use_fused = True
    span = (t("far") - t("near")).reshape(B, 1, 1)

    def rel(got, ref):
        got = got.cpu().double().numpy().reshape(ref.shape)
        return float(np.abs(got - ref).max()) / float(np.abs(ref).max())

    e = {"eikonal:fused": rel(grad * 2 / span, g["eikonal"]),
         "eikonal:module": rel(m_grad * 2 / span, g["eikonal"]),
         "sdf:fused": rel(sdf, g["sdf"]), "sdf:module": rel(m_sdf, g["sdf"]),
         "sdf:query": rel(q_sdf, g["sdf"])}
    for k, v in e.items():
        _record[f"siren_eikonal_fixture:{k}"] = v
    print("eikonal_siren.npz, max |err| / max |ref|:", e)
    assert e["eikonal:fused"] <= REL_EIKONAL
    assert e["sdf:fused"] <= REL_SDF and e["sdf:query"] <= REL_SDF


# ---------------------------------------------------------------------------- 10
@pytest.mark.parametrize("scale", [4.0, 0.25])
def test_gradient_dynamic_range(ren, ren64, lat, scale):
    """10. Latents x4 (gamma up to several times 30: the tangents grow faster per layer)
    and x0.25: finite, and the 3x rule for the gradient and both SDFs."""
    pts, dirs = _generic_points()
    tp, td = torch.from_numpy(pts).to(DEV), torch.from_numpy(dirs).to(DEV)
    lat_s = (lat * scale).contiguous()
    ref_sdf, _, ref_grad = _ref64(ren64, pts, dirs, lat_s)
    with torch.no_grad():
        sdf, grad = ren.query_gradient(tp, lat_s)
        q_sdf, _ = ren.query(tp, lat_s, return_rgb=False)
    assert torch.isfinite(grad).all() and torch.isfinite(sdf).all()
    m_sdf, _ = _module_query(ren, tp, td, lat_s)
    name = f"siren_grad_latent_x{scale:g}"
    _check(name, grad.cpu().numpy(), _module_grad(ren, tp, lat_s), ref_grad)
    _check(f"{name}:sdf", sdf.cpu().numpy(), m_sdf, ref_sdf)
    _check(f"{name}:query_sdf", q_sdf.cpu().numpy(), m_sdf, ref_sdf)


# ---------------------------------------------------------------------------- 11
def test_gradient_several_passes_per_workgroup(ren, ren64, lat):
    """11. The launch caps the workgroups of a face at 1024 / B, so for B = 2 a workgroup
    loops over its passes only when M > 32 * 512.  M = 3 * 16384 + 37 gives every workgroup
    3 or 4 passes with a partial last pass: the weight ring running ahead across passes
    (57 units per pass: its parity alternates), the next pass's points loaded under the
    last layer.  Bit-equal to the same points in calls of one pass per workgroup, and a
    seeded subset that covers every loop iteration against float64."""
    cap = 1024 // 2
    M = 3 * GROUP * cap + 37
    rng = np.random.default_rng(23)
    pts = rng.uniform(-2.1, 2.1, (2, M, 3)).astype(np.float32)
    tp = torch.from_numpy(pts).to(DEV)
    with torch.no_grad():
        sdf, grad = ren.query_gradient(tp, lat, chunk_points=M)           # one call
        sdf1, grad1 = ren.query_gradient(tp, lat, chunk_points=GROUP * cap)
    assert grad.shape == (2, M, 3)
    assert torch.equal(grad, grad1) and torch.equal(sdf, sdf1)
    sub = np.sort(rng.choice(M, 320, replace=False))
    sub = np.union1d(sub, [0, GROUP * cap - 1, GROUP * cap, 3 * GROUP * cap, M - 1])
    its = (sub // GROUP) // cap                             # the workgroup's loop iteration
    assert set(its.tolist()) == {0, 1, 2, 3}
    ps = np.ascontiguousarray(pts[:, sub])
    _, _, ref = _ref64(ren64, ps, np.zeros_like(ps), lat)
    module = _module_grad(ren, tp[:, sub].contiguous(), lat)
    got = grad[:, sub].cpu().numpy()
    _check("siren_grad_passes", got, module, ref)
    for k in range(4):
        sel = its == k
        _check(f"siren_grad_passes_it{k}", got[:, sel], module[:, sel], ref[:, sel])


# ---------------------------------------------------------------------------- 12
def test_chunking_and_repeats_are_bitwise_neutral(ren, lat):
    """12. chunk_groups / chunk_points do not change a bit; nor does calling twice."""
    torch.manual_seed(2)
    pts = torch.rand(2, 32 * 40 + 5, 3, device=DEV) * 4.2 - 2.1
    d = F.normalize(torch.randn(2, 3, device=DEV), dim=-1)
    dp = F.normalize(torch.randn(2, pts.shape[1], 3, device=DEV), dim=-1)
    with torch.no_grad():
        sdf1, rgb1 = ren.query(pts, lat, viewdirs=d)
        sdf2, rgb2 = ren.query(pts, lat, viewdirs=d)
        sdf3, rgb3 = ren.query(pts, lat, viewdirs=d, chunk_groups=16)
        p1 = ren.query(pts, lat, viewdirs=dp)
        p3 = ren.query(pts, lat, viewdirs=dp, chunk_groups=400)
        gs1, g1 = ren.query_gradient(pts, lat)
        gs2, g2 = ren.query_gradient(pts, lat)
        gs3, g3 = ren.query_gradient(pts, lat, chunk_points=64)
    assert torch.equal(sdf1, sdf2) and torch.equal(rgb1, rgb2)
    assert torch.equal(sdf1, sdf3) and torch.equal(rgb1, rgb3)
    assert torch.equal(p1[0], p3[0]) and torch.equal(p1[1], p3[1]) and torch.equal(p1[0], sdf1)
    assert torch.equal(gs1, gs2) and torch.equal(g1, g2)
    assert torch.equal(gs1, gs3) and torch.equal(g1, g3)
    # the packings are cached per weight version, the gradient's in an entry of its own
    assert ren._pack_cache[1].data_ptr() != ren._grad_pack_cache[1].data_ptr()
    with torch.no_grad():
        with pytest.raises(ValueError, match="encode_only"):
            ren.query_gradient(pts, lat, encode_only=True)


# ---------------------------------------------------------------------------- 13
def test_mesh_helpers_run_fused(sdfr, ren, lat, tmp_path):
    """13. sdf_cube -> marching cubes -> color_mesh, normal_mesh on the fused path."""
    lat1 = lat[:1]
    res = 16
    with torch.no_grad():
        assert ren._query_fused_ok(sdfr.cube_points(res, DEV).reshape(1, -1, 3), lat1)
        cube = sdfr.sdf_cube(ren, lat1, res=res)
    assert cube.shape == (1, res, res, res, 1)
    below = float((cube < 0).float().mean())
    assert 0.2 < below < 0.9, below                         # the level set exists
    mesh = sdfr.extract_mesh_with_marching_cubes(cube)
    V = len(mesh.vertices)
    assert V > 0
    col = sdfr.color_mesh(mesh, ren, lat1)
    assert col.shape == (V, 3) and col.min() >= 0.0 and col.max() <= 1.0
    n = sdfr.normal_mesh(mesh, ren, lat1)
    assert n.shape == (V, 3)
    np.testing.assert_allclose(np.linalg.norm(n, axis=-1), 1.0, rtol=0, atol=1e-6)
    v = sdfr.world_to_network(torch.from_numpy(mesh.vertices).to(DEV)).unsqueeze(0)
    module = _module_grad(ren, v, lat1)[0].astype(np.float64)
    gmin = float(np.linalg.norm(module, axis=-1).min())
    assert gmin > 0
    m_unit = module / np.linalg.norm(module, axis=-1, keepdims=True)
    # first-order propagation of the gradient's max-error bound through g / |g|
    bound = 3 * MEASURED_MAX["siren_grad_points"] / gmin
    err = float(np.abs(n - m_unit).max())
    _record["siren_mesh:normal_vs_module"] = [err, bound, gmin]
    print(f"normals vs module path: max {err:.3e} (bound {bound:.3e}, min |grad| {gmin:.3e})")
    assert err <= bound
    res_e = sdfr.eikonal_residual(ren, lat1, v)
    assert res_e.shape == (1, V) and torch.isfinite(res_e).all()
    lines = mesh.export(str(tmp_path / "siren.obj")).splitlines()
    vl = [ln for ln in lines if ln.startswith("v ")]
    assert len(vl) == V and all(len(ln.split()) == 7 for ln in vl)
    assert sum(ln.startswith("vn ") for ln in lines) == V
    fl = [ln for ln in lines if ln.startswith("f ")]
    assert fl and all(all(p.split("//")[0] == p.split("//")[1] for p in ln.split()[1:])
                      for ln in fl)


# ---------------------------------------------------------------------------- 14
def test_generator_calls_equal_renderer_calls(sdfr):
    """14. Generator.query_field / query_field_gradient on a SIREN generator = forward's
    mapping network and truncation, then the renderer-level calls, bit for bit."""
    opt = sdfr.vol_render_opt(ngp=False)
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    assert g.renderer._net_kind() == 1
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
    assert want_g[1].abs().max() > 0

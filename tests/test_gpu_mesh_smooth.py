"""GPU: mesh smoothing (csrc/mesh_smooth.hip, mesh.smooth_mesh / mesh_boundary, sparse_mesh /
extract_mesh_sparse(smooth=...)) against the NumPy definition of tests/mesh_smooth_ref.py.
Every output is a pure function of the mesh, the lattice and the weights, so every comparison
is assert_array_equal; the vertices are compared through their bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R
from tests import mesh_smooth_ref as M
from tests.mesh_smooth_ref import HAND_MADE, NONE, UNIT, one_triangle, two_triangles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


# ------------------------------------------------------------------------------- helpers
def _dev(verts, faces, dtype=torch.int32):
    return (torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(faces, np.int64).reshape(-1, 3)).to(DEV, dtype))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _gpu(sdfr, verts, faces, dtype=torch.int32, **kw):
    out = sdfr.smooth_mesh(*_dev(verts, faces, dtype), **kw)
    torch.cuda.synchronize()
    assert isinstance(out, sdfr.Smoothed) and all(t.is_cuda for t in out)
    assert out.verts.dtype == torch.float32 and out.verts.shape == (len(verts), 3)
    assert out.valence.dtype == torch.int32 and out.boundary.dtype == torch.bool
    return {k: t.cpu().numpy() for k, t in zip(out._fields, out)}


def _check(sdfr, verts, faces, origin, unit_log2, iterations=3, lam=0.5, mu=-0.53, pin=True):
    want = M.smooth(verts, faces, M.schedule(iterations, lam, mu), origin, unit_log2, pin)
    got = _gpu(sdfr, verts, faces, iterations=iterations, lam=lam, mu=mu, pin_boundary=pin,
               origin=tuple(float(x) for x in origin), unit_log2=unit_log2)
    np.testing.assert_array_equal(got["valence"], want["valence"])
    np.testing.assert_array_equal(got["boundary"], want["boundary"])
    np.testing.assert_array_equal(_bits(got["verts"]), _bits(want["verts"]))
    return got, want


def _box(verts):
    return M.lattice(verts.min(0), verts.max(0))


def _two_body(sdfr):
    """marching_cubes of the two-body volume at 64^3: 7110 vertices (four scan tiles, 28
    workgroups), 14212 faces, closed."""
    if "mesh" not in _cache:
        v, f = sdfr.marching_cubes(torch.from_numpy(R.two_body(R.grid_points(64))).to(DEV), 0.0)
        _cache["mesh"] = (v.cpu().numpy(), f.cpu().numpy().astype(np.int64))
    return _cache["mesh"]


def _raw(sdfr, verts, faces, weights, origin, unit_log2, pin=1, short_ws=0, runs=1):
    """The two C calls themselves -> (rc of prepare, [(rc of run, verts_out)])."""
    L = sdfr._lib
    lib = L.lib()
    v, f = _dev(verts, faces)
    V, F = len(v), len(f)
    n = lib.sdfr_mesh_smooth_workspace_bytes(V, F)
    ws = torch.zeros(n, dtype=torch.uint8, device=DEV)
    rc = lib.sdfr_mesh_smooth_prepare(L.ptr(v), L.ptr(f), V, F, *origin, unit_log2, pin,
                                      L.ptr(ws), n - short_ws, None, None, None)
    outs = []
    w = (ctypes.c_float * max(len(weights), 1))(*weights)
    for _ in range(runs):
        out = torch.full((V, 3), -7.0, device=DEV)
        r = lib.sdfr_mesh_smooth_run(L.ptr(v), V, w, len(weights), L.ptr(ws), n - short_ws,
                                     L.ptr(out), None)
        torch.cuda.synchronize()
        outs.append((r, out.cpu().numpy()))
    return rc, outs, L


# ----------------------------------------------------------------- 1. the hand-made cases
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_meshes(sdfr, name):
    v, f = HAND_MADE[name]()
    for pin in (True, False):
        for it, mu in ((1, None), (1, -0.53), (4, -0.53), (0, None)):
            _check(sdfr, v, f, **UNIT, iterations=it, mu=mu, pin=pin)
        _check(sdfr, v, f, *_box(v), iterations=3, pin=pin)


def test_one_triangle_pinned_and_ties_to_even(sdfr):
    v, f = one_triangle()
    got, _ = _check(sdfr, v, f, **UNIT, iterations=1, mu=None, pin=True)
    np.testing.assert_array_equal(_bits(got["verts"]), _bits(v))
    assert got["boundary"].all() and got["valence"].tolist() == [1, 1, 1]
    got, _ = _check(sdfr, v, f, **UNIT, iterations=1, mu=None, pin=False)
    assert got["verts"][:, 0].tolist() == [10.0, 11.0, 10.0]     # D = 2: 0.5 -> 0
    assert got["verts"][:, 1].tolist() == [12.0, 12.0, 12.0]     # D = 6: 1.5 -> 2, -1.5 -> -2


def test_unreferenced_vertex_no_faces_and_one_vertex(sdfr):
    v, f = HAND_MADE["repeated"]()
    got, _ = _check(sdfr, v, f, **UNIT, iterations=2, pin=False)
    assert got["valence"].tolist() == [2, 3, 3, 2, 2, 0]
    np.testing.assert_array_equal(_bits(got["verts"][5]), _bits(v[5]))
    assert (got["verts"][:5] != v[:5]).any()
    got, _ = _check(sdfr, np.float32([[1.25, 2, 3], [4, 5.5, 6]]), NONE, **UNIT, pin=False)
    assert not got["boundary"].any() and got["valence"].tolist() == [0, 0]
    got, _ = _check(sdfr, np.float32([[3, 1, 2]]), np.int64([[0, 0, 0]]), **UNIT, pin=False)
    assert got["valence"].tolist() == [3] and got["verts"].tolist() == [[3.0, 1.0, 2.0]]


# ---------------------------------------------------------------------------- 2. the clamp
def test_state_stops_at_the_clamp(sdfr):
    """A vertex at q = 2^30 and 40 passes of weight -1: the differences double every pass, so
    the state runs into both ends of the clamp; no integer overflow."""
    v = np.float32([[0, 0, 0], [2.0 ** 30, 0, 3], [2.0 ** 30, 2.0 ** 29, 0], [0, 2.0 ** 30, 5]])
    _, f = two_triangles()
    want = M.smooth(v, f, [-1.0] * 40, (0, 0, 0), 0, pin_boundary=False)
    assert want["q"].min() == -2 ** 30 and want["q"].max() == 2 ** 31 - 1
    # (the Python call has no negative lam: the C call takes the weights as they are)
    rc, outs, _ = _raw(sdfr, v, f, [-1.0] * 40, (0.0, 0.0, 0.0), 0, pin=0)
    assert rc == 0 and outs[0][0] == 0
    np.testing.assert_array_equal(_bits(outs[0][1]), _bits(want["verts"]))
    assert outs[0][1].min() == -2.0 ** 30 and outs[0][1].max() == 2.0 ** 31


# ------------------------------------------------------------------------- 3. long rows
def test_fan_hub_row_of_thousands(sdfr):
    v, f = R.fan(8192)
    got, want = _check(sdfr, v, f, *_box(v), iterations=3, pin=False)
    assert got["valence"][-1] == 8192 and got["valence"].max() == 8192
    assert got["boundary"].all()                     # every rim edge {i, i + 1} has one face
    assert (got["verts"] != v).any(1).mean() > 0.9
    got, _ = _check(sdfr, v, f, *_box(v), iterations=3, pin=True)
    np.testing.assert_array_equal(_bits(got["verts"]), _bits(v))
    # two fans over one closed rim (a double cone, closed): nothing is pinned, two long rows
    n = 8192
    i = np.arange(n, dtype=np.int64)
    j = (i + 1) % n
    g = np.concatenate([np.stack([np.full(n, n), i, j], 1), np.stack([np.full(n, n + 1), j, i], 1)])
    got, _ = _check(sdfr, v, g, *_box(v), iterations=3, pin=True)
    assert not got["boundary"].any() and got["valence"].tolist() == [4] * n + [n, n]
    val, bnd = sdfr.mesh_boundary(*_dev(v, f))
    np.testing.assert_array_equal(val.cpu().numpy(), want["valence"])
    np.testing.assert_array_equal(bnd.cpu().numpy(), want["boundary"])


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65, 100, 129])
def test_fans_about_the_long_row_cut_off(sdfr, n):
    """The hub's row has n corners: up to 32 its own lane walks it, from 33 on the whole wave,
    in steps of 64 corners whose last one is partial unless 64 divides n."""
    v, f = R.fan(n)
    got, _ = _check(sdfr, v, f, *_box(v), iterations=3, pin=False)
    assert got["valence"][-1] == n and got["valence"][:-1].max() == 2
    # several hubs in one wave, each with another valence: vertices 0..5 are hubs of disjoint fans
    parts, base = [], 6
    for hub, m in enumerate((n, 33, 7, 100, n + 1, 40)):
        i = base + np.arange(m, dtype=np.int64)
        parts.append(np.stack([np.full(m, hub), i, i + 1], 1))
        base += m + 1
    g = np.concatenate(parts)
    w = R.positions(base, 6)
    got, _ = _check(sdfr, w, g, *_box(w), iterations=3, pin=False)
    assert got["valence"][:6].tolist() == [n, 33, 7, 100, n + 1, 40]


# -------------------------------------------------------- 4. many workgroups, closed mesh
def test_two_body_mesh_closed(sdfr):
    v, f = _two_body(sdfr)
    assert (len(v), len(f)) == (7110, 14212)
    got, _ = _check(sdfr, v, f, *_box(v), iterations=5)
    assert got["boundary"].sum() == 0
    np.testing.assert_array_equal(got["valence"], np.bincount(f.ravel(), minlength=len(v)))
    assert (got["verts"] != v).any(1).mean() > 0.9
    # the default lattice is that of the bounding box
    out = sdfr.smooth_mesh(*_dev(v, f, torch.int64), iterations=5)
    np.testing.assert_array_equal(_bits(out.verts.cpu().numpy()), _bits(got["verts"]))


# ---------------------------------------------------------- 5. many workgroups, open mesh
@pytest.mark.parametrize("pin", [True, False])
def test_height_field_patch_open(sdfr, pin):
    v, f = M.patch(96)
    assert len(v) == 9216
    got, _ = _check(sdfr, v, f, *_box(v), iterations=4, pin=pin)
    assert int(got["boundary"].sum()) == 380
    b = got["boundary"]
    if pin:
        np.testing.assert_array_equal(_bits(got["verts"][b]), _bits(v[b]))
    else:
        assert (got["verts"][b] != v[b]).any(1).all()
    _check(sdfr, v, f, *_box(v), iterations=6, lam=0.25, mu=None, pin=pin)    # Laplacian
    _check(sdfr, v, f, *_box(v), iterations=3, lam=1.0, mu=0, pin=pin)


# ------------------------------------------------------------------- 6. order freedom
def test_renumbered_and_shuffled_mesh_gives_the_permuted_bits(sdfr):
    v, f = _two_body(sdfr)
    origin, ul = _box(v)
    plain, _ = _check(sdfr, v, f, origin, ul, iterations=4)
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(v))
    pv, pf = R.renumber(v, f, perm)
    pf = pf[rng.permutation(len(pf))][:, [1, 2, 0]]
    got, _ = _check(sdfr, pv, pf, origin, ul, iterations=4)
    np.testing.assert_array_equal(_bits(got["verts"][perm]), _bits(plain["verts"]))
    np.testing.assert_array_equal(got["valence"][perm], plain["valence"])
    again = _gpu(sdfr, pv, pf, iterations=4, origin=tuple(map(float, origin)), unit_log2=ul)
    np.testing.assert_array_equal(_bits(again["verts"]), _bits(got["verts"]))


# --------------------------------------------------------------------------- 7. errors
def test_bad_inputs_are_value_errors(sdfr):
    v, f = _two_body(sdfr)
    origin, ul = _box(v)
    lat = dict(origin=tuple(map(float, origin)), unit_log2=ul)
    for bad in (len(v), -3, 2 ** 31 - 1):
        g = f.copy()
        g[777, 1] = bad
        with pytest.raises(ValueError, match=r"outside \[0, V\)"):
            sdfr.smooth_mesh(*_dev(v, g), **lat)
        with pytest.raises(ValueError, match=r"outside \[0, V\)"):
            sdfr.mesh_boundary(*_dev(v, g))
    for bad in (float("nan"), float("inf")):
        w = v.copy()
        w[4321, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            sdfr.smooth_mesh(*_dev(w, f), **lat)                  # found by the kernel
        with pytest.raises(ValueError, match="not finite"):
            sdfr.smooth_mesh(*_dev(w, f))                         # found with the bounding box
    w = v.copy()
    w[5, 0] = v[:, 0].min() - 1.0
    with pytest.raises(ValueError, match="outside the lattice"):
        sdfr.smooth_mesh(*_dev(w, f), **lat)
    with pytest.raises(ValueError, match="outside the lattice"):
        sdfr.smooth_mesh(*_dev(v, f), origin=lat["origin"], unit_log2=ul - 2)
    for kw in (dict(iterations=-1), dict(iterations=2.5), dict(iterations=True), dict(lam=0.0),
               dict(lam=1.5), dict(mu=0.1), dict(mu=-1.5), dict(lam=float("nan")),
               dict(origin=(0, 0, 0)), dict(unit_log2=-20), dict(iterations=600),
               dict(origin=(0, 0, 0), unit_log2=97), dict(origin=(0, 0, 0), unit_log2=-127)):
        with pytest.raises(ValueError):
            sdfr.smooth_mesh(*_dev(v, f), **kw)
    torch.cuda.synchronize()
    _check(sdfr, v, f, origin, ul, iterations=1)                  # the device is fine


def test_c_calls_reject_before_any_launch_and_rerun(sdfr):
    v, f = _two_body(sdfr)
    origin, ul = _box(v)
    o = tuple(map(float, origin))
    w = [0.5, -0.53] * 2
    want = M.smooth(v, f, w, origin, ul)["verts"]
    rc, outs, L = _raw(sdfr, v, f, w, o, ul, runs=2)
    assert rc == 0 and [r for r, _ in outs] == [0, 0]
    for _, out in outs:                                           # each run starts from prepare
        np.testing.assert_array_equal(_bits(out), _bits(want))
    for weights in ([0.5, 1.5], [0.5, float("nan")], [-1.0000001], [0.5] * 1025):
        rc, outs, _ = _raw(sdfr, v, f, weights, o, ul)
        assert rc == 0 and outs[0][0] == L.SDFR_EINVAL
        assert (outs[0][1] == -7.0).all()                         # nothing written
    rc, outs, _ = _raw(sdfr, v, f, w, o, ul, short_ws=1)
    assert rc == L.SDFR_EINVAL and b"workspace" in L.lib().sdfr_last_error()
    rc, outs, _ = _raw(sdfr, v, f, w, o, 97)
    assert rc == L.SDFR_EINVAL
    rc, outs, _ = _raw(sdfr, v, f, w, (float("inf"), 0.0, 0.0), ul)
    assert rc == L.SDFR_EINVAL
    lib = L.lib()
    assert lib.sdfr_mesh_smooth_workspace_bytes(0, 0) == 0
    assert lib.sdfr_mesh_smooth_workspace_bytes(2 ** 31, 0) == 0
    assert lib.sdfr_mesh_smooth_workspace_bytes(10, 2 ** 31 // 3 + 1) == 0
    dv, _ = _dev(v, f)
    ws = torch.zeros(lib.sdfr_mesh_smooth_workspace_bytes(len(v), len(f)), dtype=torch.uint8,
                     device=DEV)
    one = (ctypes.c_float * 1)(0.5)
    assert lib.sdfr_mesh_smooth_run(L.ptr(dv), len(v), one, 1, L.ptr(ws), 64, L.ptr(dv),
                                    None) == L.SDFR_EINVAL       # a short workspace
    assert lib.sdfr_mesh_smooth_run(L.ptr(dv), len(v), one, 1, L.ptr(ws), ws.numel(),
                                    L.ptr(dv), None) == L.SDFR_EINVAL    # verts_out = verts
    assert lib.sdfr_mesh_smooth_run(L.ptr(dv), len(v), None, 1, L.ptr(ws), ws.numel(),
                                    L.ptr(ws), None) == L.SDFR_EINVAL
    # iterations = 0: the input's bits
    got = _gpu(sdfr, v, f, iterations=0)
    np.testing.assert_array_equal(_bits(got["verts"]), _bits(v))


# ------------------------------------------------------------------------- 8. plumbing
def _sparse_sphere(sdfr, res):
    c = sdfr.cube_axis(res, DEV)
    axes = (c, c, c)

    def evaluate(p):
        return p.norm(dim=-1) - R.SPHERE_RADIUS

    mid = torch.arange(res // 8, device=DEV) * 8 + 4
    centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"), -1)
    seeds = evaluate(centres.reshape(-1, 3)).abs() <= 4 * 3 ** 0.5 * 2 / res      # L = 1
    return evaluate, axes, seeds


def _scaled(verts, res):
    verts = verts.clone()
    for axis in range(3):
        verts[:, axis] = (verts[:, axis] / float(res) - 0.5) * 0.24
    verts[:, 2] *= -1
    verts[:, 1] *= -1
    return verts.cpu().numpy()


def test_sparse_mesh_smooths_after_simplify_and_before_the_copy(sdfr):
    res = 64
    evaluate, axes, seeds = _sparse_sphere(sdfr, res)
    verts, faces, _ = sdfr.sparse_extract(evaluate, axes, res, seeds)
    plain = sdfr.sparse_mesh(evaluate, axes, res, seeds)[0]
    none = sdfr.sparse_mesh(evaluate, axes, res, seeds, smooth=None)[0]
    for m in (plain, none):                                       # smooth=None: today's path
        np.testing.assert_array_equal(_bits(m.vertices), _bits(_scaled(verts, res)))
        np.testing.assert_array_equal(m.faces, faces.cpu().numpy())
    kv, kf, _ = sdfr.keep_components(verts, faces, largest=1)
    s = sdfr.simplify_mesh(kv, kf, cell=2.0, origin=(0, 0, 0), dims=(32, 32, 32))
    origin, ul = sdfr.smooth_lattice((0, 0, 0), (res, res, res))
    assert (origin, ul) == ((0.0, 0.0, 0.0), -23)
    sm = sdfr.smooth_mesh(s.verts, s.faces, iterations=3, origin=origin, unit_log2=ul)
    want = M.smooth(s.verts.cpu().numpy(), s.faces.cpu().numpy(), M.schedule(3), origin, ul)
    np.testing.assert_array_equal(_bits(sm.verts.cpu().numpy()), _bits(want["verts"]))
    mesh = sdfr.sparse_mesh(evaluate, axes, res, seeds, components={"largest": 1}, simplify=2,
                            smooth=3)[0]
    np.testing.assert_array_equal(_bits(mesh.vertices), _bits(_scaled(sm.verts, res)))
    np.testing.assert_array_equal(mesh.faces, s.faces.cpu().numpy())
    as_dict = sdfr.sparse_mesh(evaluate, axes, res, seeds, components={"largest": 1},
                               simplify=2, smooth={"iterations": 3, "mu": -0.53})[0]
    np.testing.assert_array_equal(_bits(as_dict.vertices), _bits(mesh.vertices))
    for bad in (True, 2.5, -1, "3", {"origin": (0, 0, 0), "unit_log2": 0}, {"lam": 2.0}):
        with pytest.raises(ValueError):
            sdfr.sparse_mesh(evaluate, axes, res, seeds, smooth=bad)


def test_generator_extract_mesh_passes_smooth_on(sdfr):
    """Generator.extract_mesh(**kw) -> extract_mesh_sparse(smooth=n) on a real field."""
    opt = sdfr.vol_render_opt(ngp=False)
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    z = torch.randn(1, 256, device=DEV)
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z])[0]
        level = float(sdfr.sdf_cube(g.renderer, lat, res=16).median())
        plain = sdfr.extract_mesh_sparse(g.renderer, lat, res=32, level=level)
        none = g.extract_mesh([z], res=32, level=level, smooth=None)
        want = sdfr.extract_mesh_sparse(g.renderer, lat, res=32, level=level, smooth=2)
        got = g.extract_mesh([z], res=32, level=level, smooth=2)
    np.testing.assert_array_equal(_bits(none.vertices), _bits(plain.vertices))
    np.testing.assert_array_equal(none.faces, plain.faces)
    np.testing.assert_array_equal(_bits(got.vertices), _bits(want.vertices))
    np.testing.assert_array_equal(got.faces, plain.faces)
    assert got.vertices.shape == plain.vertices.shape and (got.vertices != plain.vertices).any()


def test_mesh_in_mesh_out_carries_attributes(sdfr):
    v, f = _two_body(sdfr)
    rng = np.random.default_rng(5)
    col = rng.random((len(v), 3)).astype(np.float32)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    origin, ul = _box(v)
    want = M.smooth(v, f, M.schedule(2), origin, ul)
    out = sdfr.smooth_mesh(sdfr.Mesh(v, f, col, nrm), iterations=2)
    assert isinstance(out, sdfr.Mesh) and out.faces.dtype == np.int64
    np.testing.assert_array_equal(_bits(out.vertices), _bits(want["verts"]))
    np.testing.assert_array_equal(out.faces, f)
    np.testing.assert_array_equal(out.vertex_colors, col)
    np.testing.assert_array_equal(out.vertex_normals, nrm)
    plain = sdfr.smooth_mesh(sdfr.Mesh(v, f), iterations=2)
    assert plain.vertex_colors is None and plain.vertex_normals is None
    val, bnd = sdfr.mesh_boundary(sdfr.Mesh(v, f))
    assert isinstance(val, np.ndarray) and not bnd.any()
    np.testing.assert_array_equal(val, want["valence"])

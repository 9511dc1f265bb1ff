"""GPU: mesh simplification by vertex clustering (csrc/mesh_simplify.hip, mesh.simplify_mesh,
sparse_mesh / extract_mesh_sparse(simplify=...)) against the NumPy definition of
tests/mesh_simplify_ref.py.  Every output is a pure function of the mesh and the grid, so
every comparison is assert_array_equal; the new vertices are compared through their bits."""
import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R
from tests import mesh_simplify_ref as S
from tests.test_mesh_simplify import (UNIT, degenerate_only_cluster, edge_pair,
                                      loose_vertex_first, tetrahedron_in_one_cell)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


# ------------------------------------------------------------------------------- helpers
def _dev(verts, faces, dtype=torch.int32):
    return (torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(faces, np.int64).reshape(-1, 3)).to(DEV, dtype))


def _gpu(sdfr, verts, faces, origin, cell, dims, drop=True, dtype=torch.int32):
    out = sdfr.simplify_mesh(*_dev(verts, faces, dtype), cell=cell, origin=origin, dims=dims,
                             drop_unreferenced=drop)
    torch.cuda.synchronize()
    assert isinstance(out, sdfr.Simplified) and all(t.is_cuda for t in out)
    assert out.verts.dtype == torch.float32 and out.verts.shape == (len(out.index_map), 3)
    assert all(t.dtype == torch.int32 for t in out[1:])
    return {k: t.cpu().numpy() for k, t in zip(out._fields, out)}


def _assert_equal(got, want):
    np.testing.assert_array_equal(got["verts"].view(np.uint32),
                                  np.ascontiguousarray(want["verts"]).view(np.uint32))
    for k in ("faces", "index_map", "cluster", "members"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _check(sdfr, verts, faces, origin, cell, dims, drop=True):
    want = S.simplify(verts, faces, origin, cell, dims, drop)
    got = _gpu(sdfr, verts, faces, origin, cell, dims, drop)
    _assert_equal(got, want)
    return got, want


def _assert_properties(got, verts, origin, cell, dims):
    """A vertex and its cluster's position share a cell (in-grid vertices); faces have three
    distinct corners; no two faces have the same vertex set."""
    verts = np.asarray(verts, np.float32)
    lo = np.asarray(origin, np.float64)
    hi = lo + np.asarray(dims, np.float64) * float(np.float32(cell))
    inside = ((verts >= lo) & (verts <= hi)).all(1) & (got["cluster"] >= 0)
    d = np.abs(got["verts"][got["cluster"][inside]].astype(np.float64) - verts[inside])
    assert inside.any() and d.max() <= float(np.float32(cell))
    sets = S.vertex_sets(got["faces"])
    assert (sets[:, 0] < sets[:, 1]).all() and (sets[:, 1] < sets[:, 2]).all()
    assert len(np.unique(sets, axis=0)) == len(sets)
    assert got["faces"].min() >= 0 and got["faces"].max() < len(got["verts"])


def _two_body(sdfr):
    """marching_cubes of the two-body volume at 64^3: 7110 vertices (four scan tiles, 28
    workgroups), 14212 faces."""
    if "mesh" not in _cache:
        v, f = sdfr.marching_cubes(torch.from_numpy(R.two_body(R.grid_points(64))).to(DEV), 0.0)
        _cache["mesh"] = (v.cpu().numpy(), f.cpu().numpy().astype(np.int64))
    return _cache["mesh"]


def _shuffled_two_body(sdfr):
    if "shuffled" not in _cache:
        v, f = _two_body(sdfr)
        rng = np.random.default_rng(11)
        v, f = R.renumber(v, f, rng.permutation(len(v)))
        _cache["shuffled"] = (v, f[rng.permutation(len(f))])
    return _cache["shuffled"]


def _grid(res, k):
    return (0.0, 0.0, 0.0), float(k), (-(-res // k),) * 3


# ----------------------------------------------------------------- 1. the hand-made cases
def test_tetrahedron_inside_one_cell(sdfr):
    v, f = tetrahedron_in_one_cell()
    with pytest.raises(ValueError, match="too coarse"):
        sdfr.simplify_mesh(*_dev(v, f), **UNIT)
    got, _ = _check(sdfr, v, f, **UNIT, drop=False)
    assert got["members"].tolist() == [4] and got["faces"].shape == (0, 3)
    assert got["verts"].tolist() == [[0.375, 0.375, 0.375]]


@pytest.mark.parametrize("reverse_second", [False, True])
def test_duplicate_faces(sdfr, reverse_second):
    got, _ = _check(sdfr, *edge_pair(reverse_second), **UNIT)
    assert got["faces"].tolist() == [[1, 2, 0]] and got["members"].tolist() == [1, 1, 2]


def test_cell_plane_outside_loose_and_degenerate(sdfr):
    v = np.float32([[1.0, 0.5, 0.5], [-3.0, 0.5, 9.0], [3.999999, 4.0, 0.0]])
    got, _ = _check(sdfr, v, np.zeros((0, 3), np.int64), **UNIT, drop=False)
    assert got["verts"][:2].tolist() == [[1.0, 0.5, 0.5], [0.0, 0.5, 4.0]]
    got, _ = _check(sdfr, *loose_vertex_first(), **UNIT)
    assert got["index_map"].tolist() == [0, 1, 2] and got["cluster"].tolist() == [0, 1, 2, 0]
    for drop in (True, False):
        got, _ = _check(sdfr, *degenerate_only_cluster(), **UNIT, drop=drop)
    assert got["cluster"].tolist() == [0, 1, 2, 3, 3, 4]
    got = _gpu(sdfr, *degenerate_only_cluster(), **UNIT)
    assert got["cluster"].tolist() == [0, 1, 2, -1, -1, -1]


def test_position_rounding(sdfr):
    """S = 1 over m = 3 members: the fp64 quotient, product and sum, each rounded once."""
    x = [-1.0 + 3 * 0.25 + 0.25 * r for r in (0.0, 0.0, 2.0 ** -20)]
    y = [2.0 + 5 * 0.25 + 0.25 * r for r in (0.25, 0.5, 0.75)]
    v = np.float32(np.stack([x, y, [0.625] * 3], 1))
    got, _ = _check(sdfr, v, [[0, 1, 2]], (-1.0, 2.0, 0.5), 0.25, (8, 8, 8), drop=False)
    assert got["verts"][0, 0] == np.float32(-1.0 + (3.0 + 1.0 / (3.0 * 2.0 ** 20)) * 0.25)
    assert got["verts"][0, 1:].tolist() == [3.375, 0.625]


# --------------------------------------------------------------------------- 2, 3. V = 1, F = 0
def test_one_vertex_and_no_faces(sdfr):
    none = np.zeros((0, 3), np.int64)
    got, _ = _check(sdfr, np.float32([[2.25, 0.5, 3.75]]), none, **UNIT, drop=False)
    assert got["verts"].tolist() == [[2.25, 0.5, 3.75]] and got["cluster"].tolist() == [0]
    got, _ = _check(sdfr, np.float32([[2.25, 0.5, 3.75]]), [[0, 0, 0]], **UNIT, drop=False)
    assert got["faces"].shape == (0, 3)
    v = (R.positions(700, 3) * 1.5 + 2).astype(np.float32)      # some outside the 4^3 grid
    got, want = _check(sdfr, v, none, **UNIT, drop=False)
    assert 1 < want["count"] == len(got["verts"]) <= 64
    with pytest.raises(ValueError, match="too coarse"):
        sdfr.simplify_mesh(*_dev(v, none), **UNIT)


# ------------------------------------------------------------------ 4. maximal contention
def test_twenty_thousand_vertices_in_one_cell(sdfr):
    rng = np.random.default_rng(4)
    v = rng.random((20000, 3), np.float32)
    f = rng.integers(0, 20000, (5000, 3))
    got, _ = _check(sdfr, v, f, (0.0, 0.0, 0.0), 1.0, (1, 1, 1), drop=False)
    assert got["members"].tolist() == [20000] and got["index_map"].tolist() == [0]
    assert (got["cluster"] == 0).all() and got["faces"].shape == (0, 3)
    # two cells, lanes of one wave in both: the per-lane atomics
    got, _ = _check(sdfr, v, f, (0.0, 0.0, 0.0), 0.5, (2, 1, 1), drop=False)
    assert int(got["members"].sum()) == 20000 and len(got["verts"]) == 2


# ------------------------------------------------------------------------ 5. 64-bit keys
def test_every_vertex_its_own_cell_keys_above_2_32(sdfr):
    n = 5000
    i = np.arange(n)
    c = np.stack([2 ** 20 + i, (i * 7) % 1000, 2 ** 21 - 1 - i % 50], 1)
    v = (c + 0.5).astype(np.float32)
    assert (v.astype(np.float64) == c + 0.5).all()
    dims = (2 ** 21,) * 3
    key = S.cells(v, (0, 0, 0), 1.0, dims)[2]
    assert key.min() > 2 ** 32 and len(np.unique(key)) == n
    assert len(np.unique(key & 0xffffffff)) < n               # the low words alone collide
    perm = np.random.default_rng(5).permutation(n)
    f = perm[np.stack([i[:-2], i[1:-1], i[2:]], 1)]
    got, _ = _check(sdfr, v, f, (0.0, 0.0, 0.0), 1.0, dims)
    np.testing.assert_array_equal(got["faces"], f)
    np.testing.assert_array_equal(got["verts"], v)
    assert got["index_map"].tolist() == list(range(n)) and (got["members"] == 1).all()


# ------------------------------------------------------------------ 6, 10, 12. a real mesh
@pytest.mark.parametrize("k,V_out,F_out", [(2, 1571, 3134), (4, 417, 821), (8, None, None)])
def test_two_body_mesh(sdfr, k, V_out, F_out):
    v, f = _two_body(sdfr)
    assert (len(v), len(f)) == (7110, 14212)
    got, want = _check(sdfr, v, f, *_grid(64, k))
    if V_out is not None:
        assert (len(got["verts"]), len(got["faces"])) == (V_out, F_out)
    assert 0 < len(got["faces"]) < len(f) / k
    _assert_properties(got, v, *_grid(64, k))
    if k == 4:
        assert want["nondegenerate"] - len(got["faces"]) == 15        # the duplicates
        c = sdfr.mesh_components(torch.from_numpy(got["verts"]).to(DEV),
                                 torch.from_numpy(got["faces"]).to(DEV))
        assert c.count == 2 and R.components(v, f)["count"] == 2
        _check(sdfr, v, f, *_grid(64, k), drop=False)


def test_default_grid_from_the_bounding_box(sdfr):
    v, f = _two_body(sdfr)
    origin, cell, dims = sdfr.simplify_grid(v.min(0), v.max(0), cells=12)
    out = sdfr.simplify_mesh(*_dev(v, f, torch.int64), cells=12)
    got = {k: t.cpu().numpy() for k, t in zip(out._fields, out)}
    _assert_equal(got, S.simplify(v, f, origin, cell, dims))
    _assert_properties(got, v, origin, cell, dims)
    out = sdfr.simplify_mesh(*_dev(v, f), cell=cell)
    _assert_equal({k: t.cpu().numpy() for k, t in zip(out._fields, out)}, got)


# --------------------------------------------------------------- 7, 8. renumbered; twice
@pytest.mark.parametrize("k", [2, 4, 8])
def test_two_body_mesh_shuffled_and_bit_equal_across_runs(sdfr, k):
    v, f = _shuffled_two_body(sdfr)
    got, _ = _check(sdfr, v, f, *_grid(64, k))
    _assert_properties(got, v, *_grid(64, k))
    plain = _gpu(sdfr, *_two_body(sdfr), *_grid(64, k))
    assert got["faces"].shape == plain["faces"].shape           # invariant under renumbering
    assert not np.array_equal(got["index_map"], plain["index_map"])
    again = _gpu(sdfr, v, f, *_grid(64, k))
    _assert_equal(again, got)


# ------------------------------------------------------------- 9. errors on device tensors
def test_bad_face_index_and_nan_vertex_are_value_errors(sdfr):
    v, f = _shuffled_two_body(sdfr)
    grid = dict(zip(("origin", "cell", "dims"), _grid(64, 4)))
    for bad in (len(v), -3, 2 ** 31 - 1):
        g = f.copy()
        g[777, 1] = bad
        with pytest.raises(ValueError, match=r"outside \[0, V\)"):
            sdfr.simplify_mesh(*_dev(v, g), **grid)
        with pytest.raises(ValueError, match=r"outside \[0, V\)"):
            sdfr.simplify_mesh(*_dev(v, g, torch.int64), **grid)
    for bad in (float("nan"), float("inf")):
        w = v.copy()
        w[4321, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            sdfr.simplify_mesh(*_dev(w, f), **grid)              # found by the kernel
        with pytest.raises(ValueError, match="not finite"):
            sdfr.simplify_mesh(*_dev(w, f), cell=4.0)            # found with the bounding box
    torch.cuda.synchronize()
    _check(sdfr, v, f, **grid)                                   # the device is fine


# ------------------------------------------------------ 11. before the copy to the host
def _sparse_two_body(sdfr, res):
    c = sdfr.cube_axis(res, DEV)
    axes = (c, c, c)
    centre = torch.tensor(R.BALL_CENTRE, device=DEV)

    def evaluate(p):
        return torch.minimum(p.norm(dim=-1) - R.SPHERE_RADIUS,
                             (p - centre).norm(dim=-1) - R.BALL_RADIUS)

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


def test_sparse_mesh_simplifies_after_the_filter_and_before_the_copy(sdfr):
    res = 128
    evaluate, axes, seeds = _sparse_two_body(sdfr, res)
    verts, faces, _ = sdfr.sparse_extract(evaluate, axes, res, seeds)
    # simplify=None: today's path
    plain = sdfr.sparse_mesh(evaluate, axes, res, seeds)[0]
    none = sdfr.sparse_mesh(evaluate, axes, res, seeds, simplify=None)[0]
    for m in (plain, none):
        np.testing.assert_array_equal(m.vertices, _scaled(verts, res))
        np.testing.assert_array_equal(m.faces, faces.cpu().numpy())
    # filter, then simplify on the grid of res and k alone, then scale
    kv, kf, _ = sdfr.keep_components(verts, faces, largest=1)
    s = sdfr.simplify_mesh(kv, kf, cell=4.0, origin=(0, 0, 0), dims=(32, 32, 32))
    _assert_equal({k: t.cpu().numpy() for k, t in zip(s._fields, s)},
                  S.simplify(kv.cpu().numpy(), kf.cpu().numpy(), (0, 0, 0), 4.0, (32, 32, 32)))
    mesh = sdfr.sparse_mesh(evaluate, axes, res, seeds, components={"largest": 1}, simplify=4)[0]
    np.testing.assert_array_equal(mesh.vertices, _scaled(s.verts, res))
    np.testing.assert_array_equal(mesh.faces, s.faces.cpu().numpy())
    assert mesh.faces.dtype == np.int64 and 0 < len(mesh.faces) < len(kf) / 4
    assert R.components(mesh.vertices, mesh.faces)["count"] == 1
    both = sdfr.sparse_mesh(evaluate, axes, res, seeds, simplify=4)[0]
    assert R.components(both.vertices, both.faces)["count"] == 2
    assert len(both.faces) > len(mesh.faces)


def test_generator_extract_mesh_passes_simplify_on(sdfr):
    """Generator.extract_mesh(**kw) -> extract_mesh_sparse(simplify=k) on a real field."""
    opt = sdfr.vol_render_opt(ngp=False)
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    z = torch.randn(1, 256, device=DEV)
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z])[0]
        level = float(sdfr.sdf_cube(g.renderer, lat, res=16).median())
        plain = sdfr.extract_mesh_sparse(g.renderer, lat, res=32, level=level)
        none = g.extract_mesh([z], res=32, level=level, simplify=None)
        want = sdfr.extract_mesh_sparse(g.renderer, lat, res=32, level=level, simplify=2)
        got = g.extract_mesh([z], res=32, level=level, simplify=2)
    np.testing.assert_array_equal(none.vertices, plain.vertices)
    np.testing.assert_array_equal(none.faces, plain.faces)
    np.testing.assert_array_equal(got.vertices, want.vertices)
    np.testing.assert_array_equal(got.faces, want.faces)
    assert 0 < len(got.faces) < len(plain.faces) and len(got.vertices) < len(plain.vertices)
    # a mean lies in its members' box, up to the quantisation (2^-20 of a cell of 2 index
    # units, 0.24 / 32 world units each) and fp32 rounding at 32 index units: below 1e-7
    assert (got.vertices >= plain.vertices.min(0) - 1e-7).all()
    assert (got.vertices <= plain.vertices.max(0) + 1e-7).all()
    sets = S.vertex_sets(got.faces)
    assert (sets[:, 0] < sets[:, 1]).all() and (sets[:, 1] < sets[:, 2]).all()
    assert len(np.unique(sets, axis=0)) == len(sets) and sets.max() < len(got.vertices)


# ------------------------------------------------------------------ 13. Mesh in, Mesh out
def test_mesh_in_mesh_out_carries_attributes_by_index_map(sdfr):
    v, f = _shuffled_two_body(sdfr)
    rng = np.random.default_rng(5)
    col = rng.random((len(v), 3)).astype(np.float32)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    origin, cell, dims = _grid(64, 4)
    want = S.simplify(v, f, origin, cell, dims)
    out = sdfr.simplify_mesh(sdfr.Mesh(v, f, col, nrm), cell=cell, origin=origin, dims=dims)
    assert isinstance(out, sdfr.Mesh) and out.faces.dtype == np.int64
    np.testing.assert_array_equal(out.vertices.view(np.uint32), want["verts"].view(np.uint32))
    np.testing.assert_array_equal(out.faces, want["faces"])
    np.testing.assert_array_equal(out.vertex_colors, col[want["index_map"]])
    np.testing.assert_array_equal(out.vertex_normals, nrm[want["index_map"]])
    plain = sdfr.simplify_mesh(sdfr.Mesh(v, f), cell=cell, origin=origin, dims=dims)
    assert plain.vertex_colors is None and plain.vertex_normals is None
    assert plain.export().count("\nf ") == len(out.faces)

"""GPU: mesh connected components (csrc/mesh_cc.hip, mesh.label_components /
component_stats / mesh_components / keep_components, extract_mesh_sparse(components=...))
against the NumPy definition of tests/mesh_cc_ref.py.  Labels, ids, counts, bounding boxes
and selections are compared with assert_array_equal: they are pure functions of the mesh.
The area is held to the bound include/sdfr.h derives from area_unit and F."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R
from tests.test_mesh_sparse import assert_same_mesh, canonical

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


# ------------------------------------------------------------------------------- helpers
def _dev(verts, faces, dtype=torch.int32):
    return (torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(faces, np.int64).reshape(-1, 3)).to(DEV, dtype))


def _gpu(sdfr, verts, faces):
    """Everything the kernels give for a mesh, as numpy (one label call, one stats call)."""
    v, f = _dev(verts, faces)
    label, comp, count = sdfr.label_components(f, len(verts))
    nv, nf, bbox, area_q, unit = sdfr.component_stats(v, f, comp, count)
    torch.cuda.synchronize()
    assert label.dtype == torch.int32 and comp.dtype == torch.int32
    assert area_q.dtype == torch.int64 and bbox.shape == (count, 6)
    return dict(label=label.cpu().numpy(), comp=comp.cpu().numpy(), count=count,
                n_vertices=nv.cpu().numpy(), n_faces=nf.cpu().numpy(),
                bbox=bbox.cpu().numpy(), area_q=area_q.cpu().numpy(), unit=unit)


def _area_bound(unit, F):
    """include/sdfr.h: |area_q u - exact| <= Fc u / 2 + 2^11 u for the kernel (Fc <= F); the
    float64 reference adds its own evaluation (<= 2^11 u by the same argument) and the
    rounding of a sum of at most F terms each <= 2^61 u / F (<= 2^13 u): 2^14 u in all."""
    return F * unit / 2 + 2.0 ** 14 * unit


def _assert_exact(got, want, F):
    assert got["count"] == want["count"]
    for k in ("label", "comp", "n_vertices", "n_faces"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["bbox"].view(np.uint32), want["bbox"].view(np.uint32))
    unit = got["unit"]
    assert unit > 0 and np.frexp(unit)[0] == 0.5                 # a power of two
    assert (got["area_q"] >= 0).all() and int(got["area_q"].sum()) < 2 ** 62
    err = np.abs(got["area_q"].astype(np.float64) * unit - want["area"])
    print("area: unit", unit, "max error", err.max(), "bound", _area_bound(unit, F))
    assert (err <= _area_bound(unit, F)).all()


def _check(sdfr, verts, faces):
    got = _gpu(sdfr, verts, faces)
    _assert_exact(got, R.components(verts, faces), len(np.reshape(faces, (-1, 3))))
    return got


def _two_body_volume(ball_only=False, res=64):
    return R.two_body(R.grid_points(res), ball_only)


def _shuffled_two_body(sdfr):
    """Case 4's mesh: marching_cubes of the two-body volume at 64^3 (ball radius 0.1, two
    components: tests/test_mesh_components.py), vertex ids and face rows permuted."""
    if "mesh" not in _cache:
        v, f = sdfr.marching_cubes(torch.from_numpy(_two_body_volume()).to(DEV), 0.0)
        v, f = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
        rng = np.random.default_rng(11)
        v, f = R.renumber(v, f, rng.permutation(len(v)))
        f = f[rng.permutation(len(f))]
        _cache["mesh"] = (v, f, R.components(v, f))
    return _cache["mesh"]


# --------------------------------------------------------------------- 1. known answers
def test_no_faces_five_vertices(sdfr):
    v = R.positions(5)
    got = _check(sdfr, v, np.zeros((0, 3), np.int64))
    assert got["count"] == 5 and got["label"].tolist() == [0, 1, 2, 3, 4]
    assert got["n_faces"].tolist() == [0] * 5 and got["area_q"].tolist() == [0] * 5
    np.testing.assert_array_equal(got["bbox"], np.concatenate([v, v], 1))


def test_one_triangle(sdfr):
    got = _check(sdfr, np.float32([[0, 0, 0], [2, 0, 0], [0, 3, -1]]), [[0, 1, 2]])
    assert got["count"] == 1 and got["label"].tolist() == [0, 0, 0]
    assert got["bbox"].tolist() == [[0, 0, -1, 2, 3, 0]]


def test_two_interleaved_tetrahedra(sdfr):
    got = _check(sdfr, *R.two_tetrahedra())
    assert got["comp"].tolist() == [0, 1] * 4 and got["n_faces"].tolist() == [4, 4]


def test_disjoint_triangles_and_unreferenced_vertices(sdfr):
    v, f = R.disjoint_triangles(1000, 37)
    assert len(v) == 3037 and len(v) % 64 and len(v) % 256
    got = _check(sdfr, v, f)
    assert got["count"] == 1037
    assert got["n_vertices"].tolist() == [3] * 1000 + [1] * 37
    assert got["n_faces"].tolist() == [1] * 1000 + [0] * 37


# ---------------------------------------------------------------------- 2. deep chains
@pytest.mark.parametrize("order", ["reverse", "random", "bitrev"])
def test_strip_renumbered(sdfr, order):
    v, f = R.strip_renumberings(4096)[order]
    assert len(v) == 4098
    got = _check(sdfr, v, f)
    assert got["count"] == 1 and (got["label"] == 0).all() and (got["comp"] == 0).all()


# ----------------------------------------------------------------- 3. maximal contention
def test_fan_around_the_largest_index(sdfr):
    v, f = R.fan(8192)
    assert (f[:, 0] == len(v) - 1).all()
    got = _check(sdfr, v, f)
    assert got["count"] == 1 and (got["label"] == 0).all()
    assert got["n_vertices"].tolist() == [8194] and got["n_faces"].tolist() == [8192]


# ------------------------------------------------------------ 4. a real mesh, shuffled
def test_two_body_mesh_shuffled(sdfr):
    v, f, want = _shuffled_two_body(sdfr)
    assert want["count"] == 2
    got = _gpu(sdfr, v, f)
    _assert_exact(got, want, len(f))
    again = _gpu(sdfr, v, f)
    np.testing.assert_array_equal(got["area_q"], again["area_q"])
    assert got["unit"] == again["unit"]
    # the public call: device tensors stay on the device, a Mesh comes back as numpy
    dv, df = _dev(v, f, torch.int64)
    c = sdfr.mesh_components(dv, df)
    assert c.comp.is_cuda and c.count == 2 and c.area.dtype == torch.float64
    np.testing.assert_array_equal(c.comp.cpu().numpy(), want["comp"])
    np.testing.assert_array_equal(c.area.cpu().numpy(), got["area_q"] * got["unit"])
    m = sdfr.mesh_components(sdfr.Mesh(v, f))
    assert isinstance(m.comp, np.ndarray) and m.count == 2
    np.testing.assert_array_equal(m.n_faces, want["n_faces"])
    np.testing.assert_array_equal(m.bbox, want["bbox"])


# ---------------------------------------------------------------------------- 5. selection
def _assert_selection(got, want):
    gv, gf, gi = (t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(gv.view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(gf, want[1])
    np.testing.assert_array_equal(gi, want[2])


def test_selection_on_the_two_body_mesh(sdfr):
    v, f, want = _shuffled_two_body(sdfr)
    dv, df = _dev(v, f)
    comp, area, nf = want["comp"], want["area"], want["n_faces"]
    big = int(np.argmax(area))
    small = 1 - big
    assert area[big] > 20 * area[small] and nf[big] > 20 * nf[small]
    only_big = np.arange(2) == big
    cases = [
        (dict(largest=1), only_big),
        (dict(largest=1, by="faces"), only_big),
        (dict(largest=2), [True, True]),
        (dict(largest=5), [True, True]),
        (dict(min_faces=int(nf[small]) + 1), only_big),
        (dict(min_faces=int(nf[small])), [True, True]),
        (dict(min_area_frac=0.5), only_big),
        (dict(min_area_frac=0.001), [True, True]),
        (dict(keep=[bool(x) for x in ~only_big]), ~only_big),
        (dict(keep=torch.tensor(only_big).to(DEV)), only_big),
    ]
    for kw, keep in cases:
        got = sdfr.keep_components(dv, df, **kw)
        assert got[1].dtype == torch.int32 and got[2].dtype == torch.int32
        _assert_selection(got, R.select(v, f, comp, keep))
    # keep-all returns the input (no unreferenced vertices in this mesh)
    kv, kf, ki = sdfr.keep_components(dv, df, largest=2)
    assert torch.equal(kv, dv) and torch.equal(kf, df)
    assert torch.equal(ki, torch.arange(len(v), device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="no component"):
        sdfr.keep_components(dv, df, min_faces=10 ** 9)
    with pytest.raises(ValueError, match="keep must be"):
        sdfr.keep_components(dv, df, keep=[True, False, True])


def test_mesh_selection_carries_colours_and_normals(sdfr):
    v, f, want = _shuffled_two_body(sdfr)
    rng = np.random.default_rng(5)
    col = rng.random((len(v), 3)).astype(np.float32)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    mesh = sdfr.Mesh(v, f, col, nrm)
    small = int(np.argmin(want["area"]))
    out = sdfr.keep_components(mesh, keep=np.arange(2) == small)
    wv, wf, wi = R.select(v, f, want["comp"], np.arange(2) == small)
    assert isinstance(out, sdfr.Mesh) and out.faces.dtype == np.int64
    np.testing.assert_array_equal(out.vertices, wv)
    np.testing.assert_array_equal(out.faces, wf)
    np.testing.assert_array_equal(out.vertex_colors, col[wi])
    np.testing.assert_array_equal(out.vertex_normals, nrm[wi])
    same = sdfr.keep_components(mesh, largest=2)
    np.testing.assert_array_equal(same.vertices, v)
    np.testing.assert_array_equal(same.faces, f)
    np.testing.assert_array_equal(same.vertex_colors, col)
    plain = sdfr.keep_components(sdfr.Mesh(v, f), largest=1)
    assert plain.vertex_colors is None and plain.vertex_normals is None


def test_ball_alone_equals_ball_only_volume(sdfr):
    """The inverse selection (everything but the largest), then largest=1 of that: the
    ball's triangles, equal to marching_cubes of the ball-only volume bit for bit."""
    v, f, want = _shuffled_two_body(sdfr)
    dv, df = _dev(v, f)
    c = sdfr.mesh_components(dv, df)
    keep = torch.ones(c.count, dtype=torch.bool, device=DEV)
    keep[c.area.argmax()] = False
    rv, rf, _ = sdfr.keep_components(dv, df, keep=keep)
    bv, bf, _ = sdfr.keep_components(rv, rf, largest=1)
    ov, of = sdfr.marching_cubes(torch.from_numpy(_two_body_volume(ball_only=True)).to(DEV), 0.0)
    assert len(bf) == len(of) > 0 and len(bv) == len(ov)
    assert_same_mesh(canonical(bv.cpu().numpy(), bf.cpu().numpy()),
                     canonical(ov.cpu().numpy(), of.cpu().numpy()))


# ------------------------------------------------------- 6. the device path saves the copy
def _two_body_sparse(sdfr, res, **kw):
    c = sdfr.cube_axis(res, DEV)
    axes = (c, c, c)
    centre = torch.tensor(R.BALL_CENTRE, device=DEV)

    def evaluate(p):
        return torch.minimum(p.norm(dim=-1) - R.SPHERE_RADIUS,
                             (p - centre).norm(dim=-1) - R.BALL_RADIUS)

    nb = res // 8
    mid = torch.arange(nb, device=DEV) * 8 + 4
    centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"), -1)
    seeds = evaluate(centres.reshape(-1, 3)).abs() <= 4 * 3 ** 0.5 * 2 / res      # L = 1
    return sdfr.sparse_mesh(evaluate, axes, res, seeds, **kw)[0]


def test_sparse_extract_filters_before_the_copy(sdfr):
    full = _two_body_sparse(sdfr, 128)
    again = _two_body_sparse(sdfr, 128, components=None)
    np.testing.assert_array_equal(full.vertices, again.vertices)
    np.testing.assert_array_equal(full.faces, again.faces)
    ref = R.components(full.vertices, full.faces)
    assert ref["count"] == 2
    filtered = _two_body_sparse(sdfr, 128, components={"largest": 1})
    want = sdfr.keep_components(full, largest=1)
    np.testing.assert_array_equal(filtered.vertices, want.vertices)
    np.testing.assert_array_equal(filtered.faces, want.faces)
    assert 0 < len(filtered.faces) < len(full.faces)
    assert len(filtered.faces) == ref["n_faces"].max()
    copied = lambda m: m.vertices.nbytes + 4 * m.faces.size          # (int32 on the device)
    assert copied(filtered) < copied(full)


# ------------------------------------------------------------- 7. errors on device tensors
@pytest.mark.parametrize("bad", ["equal_to_V", "negative"])
def test_bad_face_index_is_a_value_error(sdfr, bad):
    """The kernel skips the face (it is never dereferenced) and the call reports it."""
    v, f = R.disjoint_triangles(200, 5)
    f = f.copy()
    f[77, 1] = len(v) if bad == "equal_to_V" else -3
    dv, df = _dev(v, f)
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(ValueError, match=r"outside \[0, V\)"):
            sdfr.mesh_components(dv, df.to(dtype))
        with pytest.raises(ValueError, match=r"outside \[0, V\)"):
            sdfr.keep_components(dv, df.to(dtype), largest=1)
    with pytest.raises(ValueError, match=r"outside \[0, V\)"):
        sdfr.label_components(df, len(v))
    torch.cuda.synchronize()
    # the device is fine: the same mesh without the bad face
    f[77] = [231, 232, 233]
    got = _check(sdfr, v, f)
    assert got["count"] == 205
    with pytest.raises(ValueError, match="does not fit|outside"):
        sdfr.mesh_components(dv, torch.full((1, 3), 2 ** 40, dtype=torch.int64, device=DEV))


def test_short_workspace_writes_nothing(sdfr):
    L = sdfr._lib
    lib = L.lib()
    v, f = R.two_tetrahedra()
    dv, df = _dev(v, f)
    n = lib.sdfr_mesh_cc_workspace_bytes(8, 8)
    ws = torch.zeros(n, dtype=torch.uint8, device=DEV)
    label = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    comp = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    count = ctypes.c_uint32(99)
    st = L.stream_of(dv)
    rc = lib.sdfr_mesh_cc_label(L.ptr(df), 8, 8, L.ptr(label), L.ptr(comp), L.ptr(ws), n - 1,
                                count, st)
    assert rc == L.SDFR_EINVAL and b"workspace too small" in lib.sdfr_last_error()
    nanf = torch.full((2, 6), float("nan"), device=DEV)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    aq = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    unit = ctypes.c_double(-1.0)
    rc = lib.sdfr_mesh_cc_stats(L.ptr(dv), L.ptr(df), L.ptr(comp), 8, 8, 2, L.ptr(cnt), L.ptr(cnt),
                                L.ptr(nanf), L.ptr(aq), unit, L.ptr(ws), n - 1, st)
    assert rc == L.SDFR_EINVAL and b"workspace too small" in lib.sdfr_last_error()
    torch.cuda.synchronize()
    assert count.value == 99 and unit.value == -1.0
    assert (label == -7).all() and (comp == -7).all() and (cnt == -7).all() and (aq == -7).all()
    assert torch.isnan(nanf).all() and not ws.any()


# --------------------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize("case", ["strip_random", "fan"])
def test_bit_equal_across_runs(sdfr, case):
    v, f = R.strip_renumberings(4096)["random"] if case == "strip_random" else R.fan(8192)
    a, b = _gpu(sdfr, v, f), _gpu(sdfr, v, f)
    for k in ("label", "comp", "n_vertices", "n_faces", "area_q"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["bbox"].view(np.uint32), b["bbox"].view(np.uint32))
    assert a["unit"] == b["unit"] and a["count"] == b["count"] == 1

"""CPU: mesh simplification by vertex clustering (include/sdfr.h "Mesh simplification",
csrc/mesh_simplify.hip, mesh.simplify_mesh): the NumPy definition of
tests/mesh_simplify_ref.py against hand-made answers and against pinned counts on marching
cubes of the two-body volume, the C ABI's names and its argument checks (fake pointers:
rejected before any launch), and the Python argument checks that need no device.
tests/test_gpu_mesh_simplify.py holds the kernels to the same helper."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R
from tests import mesh_simplify_ref as S

REPO = Path(__file__).resolve().parents[1]
FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch
NAMES = ("sdfr_mesh_simplify_workspace_bytes", "sdfr_mesh_simplify_count",
         "sdfr_mesh_simplify_emit")
UNIT = dict(origin=(0.0, 0.0, 0.0), cell=1.0, dims=(4, 4, 4))


# ------------------------------------------------------- the hand-made meshes (shared with GPU)
def tetrahedron_in_one_cell():
    v = np.float32([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [0.25, 0.75, 0.25], [0.25, 0.25, 0.75]])
    return v, np.int64([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def edge_pair(reverse_second=False):
    """Two triangles on the edge 0-1 whose far corners 2 and 3 share the cell (0, 1, 0)."""
    v = np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.25, 1.5, 0.5], [0.75, 1.25, 0.5]])
    second = [0, 1, 3] if reverse_second else [1, 0, 3]
    return v, np.int64([[1, 2, 0], second])


def loose_vertex_first():
    """Vertex 0 is referenced by nothing and shares the cell (2, 2, 2) with vertex 3."""
    v = np.float32([[2.75, 2.5, 2.5], [0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.25, 2.5, 2.5]])
    return v, np.int64([[1, 2, 3]])


def degenerate_only_cluster():
    """Face 1 = (3, 4, 5) has two corners in the cell (3, 3, 3), so it collapses; vertex 5's
    cell (0, 3, 0) is referenced by nothing else."""
    v = np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5],
                    [3.25, 3.5, 3.5], [3.75, 3.5, 3.5], [0.5, 3.5, 0.5]])
    return v, np.int64([[0, 1, 2], [3, 4, 5]])


# ------------------------------------------------------------------ the helper, by hand
def test_tetrahedron_inside_one_cell():
    v, f = tetrahedron_in_one_cell()
    s = S.simplify(v, f, **UNIT)
    assert s["count"] == 1 and s["nondegenerate"] == 0
    assert len(s["verts"]) == 0 and len(s["faces"]) == 0 and len(s["index_map"]) == 0
    assert s["cluster"].tolist() == [-1] * 4
    s = S.simplify(v, f, **UNIT, drop_unreferenced=False)
    assert s["index_map"].tolist() == [0] and s["members"].tolist() == [4]
    assert s["cluster"].tolist() == [0] * 4 and len(s["faces"]) == 0
    np.testing.assert_array_equal(s["verts"], np.float32([[0.375, 0.375, 0.375]]))


@pytest.mark.parametrize("reverse_second", [False, True])
def test_duplicate_faces_keep_the_lower_index_with_its_corner_order(reverse_second):
    v, f = edge_pair(reverse_second)
    s = S.simplify(v, f, **UNIT)
    assert s["count"] == 3 and s["nondegenerate"] == 2
    assert s["faces"].tolist() == [[1, 2, 0]]                 # face 0 as it was, either way
    assert s["index_map"].tolist() == [0, 1, 2] and s["members"].tolist() == [1, 1, 2]
    assert s["cluster"].tolist() == [0, 1, 2, 2]
    np.testing.assert_array_equal(
        s["verts"], np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.375, 0.5]]))


def test_cell_plane_and_outside_vertices():
    v = np.float32([[1.0, 0.5, 0.5],         # on the plane x = 1: the upper cell, offset 0
                    [-3.0, 0.5, 9.0],        # outside: the nearest boundary cell
                    [3.999999, 4.0, 0.0]])   # y on the outer plane: clamped to the last cell
    c, q, key = S.cells(v, **UNIT)
    assert c.tolist() == [[1, 0, 0], [0, 0, 3], [3, 3, 0]]
    assert q[0].tolist() == [0, 2 ** 19, 2 ** 19]
    assert q[1].tolist() == [0, 2 ** 19, 2 ** 20]
    assert q[2, 1] == 2 ** 20 and q[2, 2] == 0
    assert key.tolist() == [16, 3, (3 * 4 + 3) * 4]
    s = S.simplify(v, np.zeros((0, 3), np.int64), **UNIT, drop_unreferenced=False)
    np.testing.assert_array_equal(s["verts"][0], np.float32([1.0, 0.5, 0.5]))
    np.testing.assert_array_equal(s["verts"][1], np.float32([0.0, 0.5, 4.0]))
    # keys above 2^32 stay apart
    c, q, key = S.cells(np.float32([[5, 7, 9], [5, 7, 10]]), (0, 0, 0), 1.0, (2 ** 21,) * 3)
    assert key.tolist() == [(5 * 2 ** 21 + 7) * 2 ** 21 + 9, (5 * 2 ** 21 + 7) * 2 ** 21 + 10]


def test_unreferenced_small_index_vertex_becomes_the_rep():
    v, f = loose_vertex_first()
    s = S.simplify(v, f, **UNIT)
    assert s["count"] == 3 and s["index_map"].tolist() == [0, 1, 2]
    assert s["cluster"].tolist() == [0, 1, 2, 0] and s["faces"].tolist() == [[1, 2, 0]]
    assert s["members"].tolist() == [2, 1, 1]
    np.testing.assert_array_equal(s["verts"][0], np.float32([2.5, 2.5, 2.5]))


def test_cluster_with_only_degenerate_faces_is_dropped():
    v, f = degenerate_only_cluster()
    s = S.simplify(v, f, **UNIT)
    assert s["count"] == 5 and s["nondegenerate"] == 1
    assert s["faces"].tolist() == [[0, 1, 2]] and s["index_map"].tolist() == [0, 1, 2]
    assert s["cluster"].tolist() == [0, 1, 2, -1, -1, -1]
    s = S.simplify(v, f, **UNIT, drop_unreferenced=False)
    assert s["index_map"].tolist() == [0, 1, 2, 3, 5] and s["members"].tolist() == [1, 1, 1, 2, 1]
    assert s["cluster"].tolist() == [0, 1, 2, 3, 3, 4] and s["faces"].tolist() == [[0, 1, 2]]


def test_position_formula_by_hand():
    """Three members of one cell of the grid origin (-1, 2, 0.5), cell 0.25: offsets
    (0, 0, 2^-20) of the cell along x, (1/4, 1/2, 3/4) along y, all 1/2 along z."""
    origin, cell = (-1.0, 2.0, 0.5), 0.25
    x = [-1.0 + 3 * 0.25 + 0.25 * r for r in (0.0, 0.0, 2.0 ** -20)]
    y = [2.0 + 5 * 0.25 + 0.25 * r for r in (0.25, 0.5, 0.75)]
    z = [0.5 + 0.125] * 3
    v = np.float32(np.stack([x, y, z], 1))
    assert (v.astype(np.float64) == np.stack([x, y, z], 1)).all()     # exact in fp32
    c, q, _ = S.cells(v, origin, cell, (8, 8, 8))
    assert c.tolist() == [[3, 5, 0]] * 3
    assert q.tolist() == [[0, 2 ** 18, 2 ** 19], [0, 2 ** 19, 2 ** 19], [1, 3 * 2 ** 18, 2 ** 19]]
    s = S.simplify(v, [[0, 1, 2]], origin, cell, (8, 8, 8), drop_unreferenced=False)
    assert s["count"] == 1 and s["members"].tolist() == [3] and len(s["faces"]) == 0
    want = [np.float32(-1.0 + (3.0 + 1.0 / (3.0 * 2.0 ** 20)) * 0.25),      # S = 1, m = 3
            np.float32(2.0 + (5.0 + (6.0 * 2.0 ** 18) / (3.0 * 2.0 ** 20)) * 0.25),
            np.float32(0.5 + (0.0 + 0.5) * 0.25)]
    assert s["verts"].dtype == np.float32
    np.testing.assert_array_equal(s["verts"][0], np.float32(want))
    assert want[1] == np.float32(3.375) and want[2] == np.float32(0.625)


# ------------------------------------------------- known answers on the two-body volume
def _two_body_mesh(res):
    from oracle import mc
    v, f = mc.marching_cubes(R.two_body(R.grid_points(res)), 0.0)
    return np.asarray(v, np.float32), np.asarray(f, np.int64)


@pytest.mark.parametrize("res,k,V,F,V_out,F_out,nondegenerate", [
    (64, 4, 7110, 14212, 417, 821, 836),
    (64, 2, 7110, 14212, 1571, 3134, 3134),
    (32, 4, 1806, 3604, 120, 232, None),
])
def test_two_body_known_answers(res, k, V, F, V_out, F_out, nondegenerate):
    v, f = _two_body_mesh(res)
    assert (len(v), len(f)) == (V, F)
    s = S.simplify(v, f, (0, 0, 0), float(k), (-(-res // k),) * 3)
    assert (len(s["verts"]), len(s["faces"])) == (V_out, F_out)
    if nondegenerate is not None:
        assert s["nondegenerate"] == nondegenerate
    sets = S.vertex_sets(s["faces"])
    assert (sets[:, 0] < sets[:, 1]).all() and (sets[:, 1] < sets[:, 2]).all()
    assert len(np.unique(sets, axis=0)) == len(sets)
    live = s["cluster"] >= 0
    assert np.abs(s["verts"][s["cluster"][live]] - v[live]).max() <= k
    assert int(s["members"].sum()) == int(live.sum())
    if res == 64:
        assert s["count"] == V_out and live.all()              # no cluster dropped
        assert R.components(v, f)["count"] == 2
    if (res, k) == (64, 4):
        assert R.components(s["verts"], s["faces"])["count"] == 2


# ------------------------------------------------------------------------------ the C ABI
def test_names_in_binding_and_header(sdfr):
    L = sdfr._lib
    assert L.ABI_VERSION == 15
    raw = (REPO / "include" / "sdfr.h").read_text()
    assert re.search(r"Mesh simplification \(added to ABI 15 without a version step", raw)
    txt = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert re.search(r"#define\s+SDFR_ABI_VERSION\s+15\b", txt)
    for name in NAMES:
        assert name in L.EXPORTS and name in L.PROTOTYPES
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % name, txt), name
    for name in ("simplify_mesh", "Simplified", "simplify_grid"):
        assert hasattr(sdfr, name), name
    assert sdfr.Simplified._fields == ("verts", "faces", "index_map", "cluster", "members")


def _rejected(sdfr, rc, msg):
    lib = sdfr._lib.lib()
    assert rc == sdfr._lib.SDFR_EINVAL
    assert msg in lib.sdfr_last_error(), lib.sdfr_last_error()


def test_c_abi_rejects_bad_arguments_before_any_launch(sdfr):
    lib = sdfr._lib.lib()
    u32 = ctypes.c_uint32
    size = lib.sdfr_mesh_simplify_workspace_bytes
    assert size(0, 5) == 0 == size(1 << 31, 5) and size(5, (1 << 31) // 3 + 1) == 0
    assert size(5, 0) > 0 and size((1 << 31) - 1, (1 << 31) // 3) > (1 << 35)
    # two tables of >= 2 V and >= 2 F slots (12 and 4 bytes), 44 bytes per vertex, 8 per face
    assert size(3037, 1000) >= 12 * 2 * 3037 + 4 * 2 * 1000 + 44 * 3037 + 8 * 1000
    assert size(100, 50) == size(100, 50)
    n = size(100, 50)
    counts = (u32 * 3)(77, 77, 77)
    big = (1 << 64) - 1
    inf, nan = float("inf"), float("nan")
    # count: verts, faces, V, F, ox, oy, oz, cell, nx, ny, nz, drop, ws, ws_bytes, counts, stream
    good = [FAKE, FAKE, 100, 50, 0.0, 0.0, 0.0, 1.0, 4, 4, 4, 1, FAKE, n, counts, None]
    for i in (0, 1, 14):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"mesh_simplify: null")
    for V, F in ((0, 50), (1 << 31, 50), (100, (1 << 31) // 3 + 1)):
        a = list(good)
        a[2], a[3], a[13] = V, F, big
        _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"V must be in [1, 2^31)")
    for cell in (0.0, -1.0, inf, nan):
        a = list(good)
        a[7] = cell
        _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"cell must be finite and > 0")
    for i in (4, 5, 6):
        a = list(good)
        a[i] = nan
        _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"origin must be finite")
    for i in (8, 9, 10):
        for d in (0, (1 << 21) + 1):
            a = list(good)
            a[i] = d
            _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"must be in [1, 2^21]")
    a = list(good)
    a[12] = None
    _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"null workspace")
    a = list(good)
    a[13] -= 1
    _rejected(sdfr, lib.sdfr_mesh_simplify_count(*a), b"workspace too small")
    # emit: verts, faces, V, F, V_out, F_out, ws, ws_bytes, verts_out, faces_out, index_map,
    #       cluster, members, stream
    good = [FAKE, FAKE, 100, 50, 10, 5, FAKE, n, FAKE, FAKE, FAKE, FAKE, FAKE, None]
    for i in (0, 1, 8, 9, 10):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_mesh_simplify_emit(*a), b"mesh_simplify: null")
    for vo, fo in ((0, 5), (101, 5), (10, 51)):
        a = list(good)
        a[4], a[5] = vo, fo
        _rejected(sdfr, lib.sdfr_mesh_simplify_emit(*a), b"V_out must be in [1, V]")
    a = list(good)
    a[6] = None
    _rejected(sdfr, lib.sdfr_mesh_simplify_emit(*a), b"null workspace")
    a = list(good)
    a[7] -= 1
    _rejected(sdfr, lib.sdfr_mesh_simplify_emit(*a), b"workspace too small")
    a = list(good)
    a[2] = 0
    _rejected(sdfr, lib.sdfr_mesh_simplify_emit(*a), b"V must be in [1, 2^31)")
    # nothing was written to the host output
    assert list(counts) == [77, 77, 77]


# ------------------------------------------------------------------ the Python-side checks
def test_selector_checks_need_no_device(sdfr):
    v, f = edge_pair()
    mesh = sdfr.Mesh(v, f)
    with pytest.raises(ValueError, match="exactly one of cell"):
        sdfr.simplify_mesh(mesh)
    with pytest.raises(ValueError, match="exactly one of cell"):
        sdfr.simplify_mesh(mesh, cell=1.0, cells=8)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell edge must be finite"):
            sdfr.simplify_mesh(mesh, cell=bad)
        with pytest.raises(ValueError, match="cells must be a positive"):
            sdfr.simplify_mesh(mesh, cells=bad)
    for bad in ((4, 4), (0, 4, 4), (4, 4, 2 ** 21 + 1), (4, 4.5, 4)):
        with pytest.raises(ValueError, match="dims must be three integers"):
            sdfr.simplify_mesh(mesh, cell=1.0, dims=bad)
    for bad in ((0, 0), (0, 0, float("nan"))):
        with pytest.raises(ValueError, match="origin must be three finite"):
            sdfr.simplify_mesh(mesh, cell=1.0, origin=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        sdfr.simplify_mesh(torch.from_numpy(v), torch.from_numpy(f), cell=1.0)
    with pytest.raises(ValueError, match="Mesh, or vertices and faces"):
        sdfr.simplify_mesh(mesh, torch.from_numpy(f), cell=1.0)
    for bad in (1, 0, -4, 2.5, True):
        with pytest.raises(ValueError, match="simplify must be None or an integer >= 2"):
            sdfr.sparse_mesh(None, None, 64, None, simplify=bad)
        with pytest.raises(ValueError, match="simplify must be None or an integer >= 2"):
            sdfr.extract_mesh_sparse(None, torch.zeros(1, 256), res=64, simplify=bad)


def test_default_grid(sdfr):
    origin, cell, dims = sdfr.simplify_grid((-1, 0, 2), (3, 1, 2), cell=0.5)
    assert origin == (-1.0, 0.0, 2.0) and cell == 0.5 and dims == (9, 3, 1)
    origin, cell, dims = sdfr.simplify_grid((-1, 0, 2), (3, 1, 2), cells=8)
    assert cell == 0.5 and dims == (9, 3, 1)
    origin, cell, dims = sdfr.simplify_grid((0, 0, 0), (1, 1, 0.5), cells=3)
    assert cell == float(np.float32(1 / 3)) and dims == (3, 3, 2)    # fp32(1/3) > 1/3
    with pytest.raises(ValueError, match="exactly one of cell"):
        sdfr.simplify_grid((0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="no extent"):
        sdfr.simplify_grid((1, 1, 1), (1, 1, 1), cells=4)
    with pytest.raises(ValueError, match="not finite"):
        sdfr.simplify_grid((0, 0, 0), (1, float("nan"), 1), cell=1.0)
    with pytest.raises(ValueError, match="dims must be three integers"):
        sdfr.simplify_grid((0, 0, 0), (1, 1, 1), cell=1e-7)

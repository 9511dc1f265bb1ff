"""CPU: mesh connected components (include/sdfr.h "Mesh connected components",
csrc/mesh_cc.hip, mesh.mesh_components / keep_components): the NumPy definition of
tests/mesh_cc_ref.py against hand-written answers, the C ABI's names and its argument
checks (fake pointers: rejected before any launch), and the Python argument checks that
need no device.  tests/test_gpu_mesh_components.py holds the kernels to the same helper."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R

REPO = Path(__file__).resolve().parents[1]
FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch
NAMES = ("sdfr_mesh_cc_workspace_bytes", "sdfr_mesh_cc_label", "sdfr_mesh_cc_stats",
         "sdfr_mesh_cc_select_count", "sdfr_mesh_cc_select_emit")


# ------------------------------------------------------------------ the helper, by hand
def test_helper_one_triangle():
    v = np.float32([[0, 0, 0], [2, 0, 0], [0, 3, -1]])
    c = R.components(v, [[0, 1, 2]])
    assert c["label"].tolist() == [0, 0, 0] and c["comp"].tolist() == [0, 0, 0]
    assert c["count"] == 1 and c["n_vertices"].tolist() == [3] and c["n_faces"].tolist() == [1]
    assert c["bbox"].tolist() == [[0, 0, -1, 2, 3, 0]]
    # 0.5 |(2,0,0) x (0,3,-1)| = 0.5 |(0, 2, 6)| = sqrt(10)
    assert c["area"].tolist() == [pytest.approx(10 ** 0.5, rel=1e-15)]
    ov, of, im = R.select(v, [[0, 1, 2]], c["comp"], [True])
    np.testing.assert_array_equal(ov, v)
    assert of.tolist() == [[0, 1, 2]] and im.tolist() == [0, 1, 2]


def test_helper_two_interleaved_tetrahedra():
    v, f = R.two_tetrahedra()
    c = R.components(v, f)
    assert c["label"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    assert c["comp"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1] and c["count"] == 2
    assert c["n_vertices"].tolist() == [4, 4] and c["n_faces"].tolist() == [4, 4]
    np.testing.assert_array_equal(c["bbox"][0], np.r_[v[0::2].min(0), v[0::2].max(0)])
    np.testing.assert_array_equal(c["bbox"][1], np.r_[v[1::2].min(0), v[1::2].max(0)])
    # the odd tetrahedron alone: vertices 1 3 5 7 -> 0 1 2 3, its faces in their order
    ov, of, im = R.select(v, f, c["comp"], [False, True])
    assert im.tolist() == [1, 3, 5, 7]
    np.testing.assert_array_equal(ov, v[1::2])
    np.testing.assert_array_equal(of, (f[1::2] - 1) // 2)
    assert R.largest_mask([3.0, 3.0], 1).tolist() == [True, False]     # ties: the lower id


def test_helper_triangle_and_two_unreferenced_vertices():
    v = R.positions(5)
    f = [[4, 1, 3]]                         # vertices 0 and 2 are referenced by nothing
    c = R.components(v, f)
    assert c["label"].tolist() == [0, 1, 2, 1, 1]
    assert c["comp"].tolist() == [0, 1, 2, 1, 1] and c["count"] == 3
    assert c["n_vertices"].tolist() == [1, 3, 1] and c["n_faces"].tolist() == [0, 1, 0]
    np.testing.assert_array_equal(c["bbox"][0], np.r_[v[0], v[0]])
    assert c["area"][0] == 0 and c["area"][2] == 0 and c["area"][1] > 0
    ov, of, im = R.select(v, f, c["comp"], [True, True, True])
    assert im.tolist() == [1, 3, 4] and of.tolist() == [[2, 0, 1]]
    ov, of, im = R.select(v, f, c["comp"], [True, True, True], drop_unreferenced=False)
    assert im.tolist() == [0, 1, 2, 3, 4] and of.tolist() == [[4, 1, 3]]
    np.testing.assert_array_equal(ov, v)


def test_helper_chains_and_fan():
    for name, (v, f) in R.strip_renumberings(256).items():
        assert (R.labels(f, len(v)) == 0).all(), name
    v, f = R.fan(100)
    assert f[:, 0].tolist() == [101] * 100 and (R.labels(f, len(v)) == 0).all()
    perm = R.bit_reversed(4098)
    assert sorted(perm.tolist()) == list(range(4098)) and perm[:3].tolist() != [0, 1, 2]


def test_two_body_volume_is_two_components_at_64():
    """The volume of the GPU tests' cases 4 and 5: at 64^3 the CPU marching cubes gives
    exactly two components with the ball radius 0.1 as stated (3.2 grid steps), the sphere
    the larger; and the ball's part equals the ball-only volume's mesh."""
    from oracle import mc
    from tests.test_mesh_sparse import assert_same_mesh, canonical
    pts = R.grid_points(64)
    v, f = mc.marching_cubes(R.two_body(pts), 0.0)
    c = R.components(v, f)
    assert c["count"] == 2 and (c["n_faces"] > 0).all()
    assert c["area"][0] > 20 * c["area"][1]           # 36 : 1 for the exact surfaces
    assert np.unique(f).size == len(v)                # no unreferenced vertices
    bv, bf, _ = R.select(v, f, c["comp"], [False, True])
    assert_same_mesh(canonical(bv, bf),
                     canonical(*mc.marching_cubes(R.two_body(pts, ball_only=True), 0.0)))


# ------------------------------------------------------------------------------ the C ABI
def test_names_in_binding_and_header(sdfr):
    L = sdfr._lib
    assert L.ABI_VERSION == 15
    txt = re.sub(r"/\*.*?\*/", " ", (REPO / "include" / "sdfr.h").read_text(), flags=re.S)
    assert re.search(r"#define\s+SDFR_ABI_VERSION\s+15\b", txt)
    for name in NAMES:
        assert name in L.EXPORTS and name in L.PROTOTYPES
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % name, txt), name
    for name in ("mesh_components", "keep_components", "Components", "label_components",
                 "component_stats", "sparse_mesh"):
        assert hasattr(sdfr, name), name
    assert sdfr.Components._fields == ("comp", "n_vertices", "n_faces", "bbox", "area", "count")


def _rejected(sdfr, rc, msg):
    lib = sdfr._lib.lib()
    assert rc == sdfr._lib.SDFR_EINVAL
    assert msg in lib.sdfr_last_error(), lib.sdfr_last_error()


def test_c_abi_rejects_bad_arguments_before_any_launch(sdfr):
    lib = sdfr._lib.lib()
    u32 = ctypes.c_uint32
    size = lib.sdfr_mesh_cc_workspace_bytes
    assert size(0, 5) == 0 == size(1 << 31, 5) and size(5, (1 << 31) // 3 + 1) == 0
    assert size(5, 0) >= 7 * 4 + 4 and size((1 << 31) - 1, (1 << 31) // 3) > (1 << 33)
    assert size(3037, 1000) >= 4 * (3037 + 2) + 4 * (1000 + 1)
    n = size(100, 50)
    out, counts, unit = u32(77), (u32 * 2)(77, 77), ctypes.c_double(-1.0)
    big = (1 << 64) - 1
    # label: faces, V, F, label, comp, ws, ws_bytes, n_components, stream
    good = [FAKE, 100, 50, FAKE, FAKE, FAKE, n, out, None]
    for i in (0, 3, 4, 7):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_mesh_cc_label(*a), b"mesh_cc_label: null")
    for V, F in ((0, 50), (1 << 31, 50), (100, (1 << 31) // 3 + 1)):
        a = list(good)
        a[1], a[2], a[6] = V, F, big
        _rejected(sdfr, lib.sdfr_mesh_cc_label(*a), b"V must be in [1, 2^31)")
    a = list(good)
    a[5] = None
    _rejected(sdfr, lib.sdfr_mesh_cc_label(*a), b"null workspace")
    a = list(good)
    a[6] -= 1
    _rejected(sdfr, lib.sdfr_mesh_cc_label(*a), b"workspace too small")
    # stats: verts, faces, comp, V, F, C, n_vertices, n_faces, bbox, area_q, unit, ws, n, stream
    good = [FAKE, FAKE, FAKE, 100, 50, 3, FAKE, FAKE, FAKE, FAKE, unit, FAKE, n, None]
    for i in (0, 1, 2, 6, 7, 8, 9, 10):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_mesh_cc_stats(*a), b"mesh_cc_stats: null")
    for C in (0, 101):
        a = list(good)
        a[5] = C
        _rejected(sdfr, lib.sdfr_mesh_cc_stats(*a), b"C must be in [1, V]")
    a = list(good)
    a[12] -= 1
    _rejected(sdfr, lib.sdfr_mesh_cc_stats(*a), b"workspace too small")
    a = list(good)
    a[3], a[12] = 0, big
    _rejected(sdfr, lib.sdfr_mesh_cc_stats(*a), b"V must be in [1, 2^31)")
    # select_count: faces, comp, keep, V, F, C, drop, ws, n, counts, stream
    good = [FAKE, FAKE, FAKE, 100, 50, 3, 1, FAKE, n, counts, None]
    for i in (0, 1, 2, 9):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_mesh_cc_select_count(*a), b"mesh_cc_select: null")
    a = list(good)
    a[5] = 0
    _rejected(sdfr, lib.sdfr_mesh_cc_select_count(*a), b"C must be in [1, V]")
    a = list(good)
    a[8] -= 1
    _rejected(sdfr, lib.sdfr_mesh_cc_select_count(*a), b"workspace too small")
    # select_emit: verts, faces, V, F, V_out, F_out, ws, n, verts_out, faces_out, index_map, stream
    good = [FAKE, FAKE, 100, 50, 10, 5, FAKE, n, FAKE, FAKE, FAKE, None]
    for i in (0, 1, 8, 9, 10):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_mesh_cc_select_emit(*a), b"mesh_cc_select: null")
    for vo, fo in ((0, 5), (101, 5), (10, 51)):
        a = list(good)
        a[4], a[5] = vo, fo
        _rejected(sdfr, lib.sdfr_mesh_cc_select_emit(*a), b"V_out must be in [1, V]")
    a = list(good)
    a[7] -= 1
    _rejected(sdfr, lib.sdfr_mesh_cc_select_emit(*a), b"workspace too small")
    # nothing was written to the host outputs
    assert out.value == 77 and list(counts) == [77, 77] and unit.value == -1.0


# ------------------------------------------------------------------ the Python-side checks
def test_selector_checks_need_no_device(sdfr):
    v, f = R.two_tetrahedra()
    mesh = sdfr.Mesh(v, f)
    with pytest.raises(ValueError, match="exactly one"):
        sdfr.keep_components(mesh)
    with pytest.raises(ValueError, match="exactly one"):
        sdfr.keep_components(mesh, largest=1, min_faces=2)
    with pytest.raises(ValueError, match="exactly one"):
        sdfr.keep_components(mesh, keep=[True, False], min_area_frac=0.5)
    with pytest.raises(ValueError, match="by must be"):
        sdfr.keep_components(mesh, largest=1, by="volume")
    for bad in ([True] * 9, [], [[True, False]]):       # more entries than vertices; none; 2-D
        with pytest.raises(ValueError, match="keep must be"):
            sdfr.keep_components(mesh, keep=bad)
    with pytest.raises(ValueError, match="exactly one"):
        sdfr.keep_components(torch.zeros(8, 3), torch.zeros(8, 3, dtype=torch.int32))


def test_cpu_tensors_are_refused(sdfr):
    v, f = R.two_tetrahedra()
    with pytest.raises(RuntimeError, match="GPU"):
        sdfr.mesh_components(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(RuntimeError, match="GPU"):
        sdfr.keep_components(torch.from_numpy(v), torch.from_numpy(f), largest=1)
    with pytest.raises(ValueError, match="Mesh, or vertices and faces"):
        sdfr.mesh_components(sdfr.Mesh(v, f), torch.from_numpy(f))
    with pytest.raises(ValueError, match="tensors"):
        sdfr.mesh_components(torch.from_numpy(v))

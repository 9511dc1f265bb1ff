"""CPU: the definition of mesh smoothing (include/sdfr.h, "Mesh smoothing") as
tests/mesh_smooth_ref.py states it -- against a plain per-vertex transcription on the
hand-made meshes, and its properties on a noisy sphere and an open patch.  No GPU and no
library needed; tests/test_gpu_mesh_smooth.py holds csrc/mesh_smooth.hip to the same
reference."""
import math

import numpy as np
import pytest

from tests import mesh_smooth_ref as M
from tests.mesh_smooth_ref import (HAND_MADE, UNIT, one_triangle, repeated_corner, tetrahedron,
                                   two_triangles)


def loop_smooth(verts, faces, weights, origin, unit_log2, pin_boundary=True):
    """The definition, one vertex and one face corner at a time, in Python integers."""
    verts = np.asarray(verts, np.float32)
    V = len(verts)
    faces = [tuple(int(x) for x in f) for f in np.asarray(faces).reshape(-1, 3)]
    u = 2.0 ** unit_log2
    o = [float(np.float32(x)) for x in origin]
    q = [[int(np.rint((float(verts[i, k]) - o[k]) / u)) for k in range(3)] for i in range(V)]
    assert all(0 <= x <= 2 ** 30 for row in q for x in row)
    d = [sum(c == i for f in faces for c in f) for i in range(V)]
    mult = {}
    for f in faces:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if a != b:
                mult[frozenset((a, b))] = mult.get(frozenset((a, b)), 0) + 1
    bnd = [any(i in e and m == 1 for e, m in mult.items()) for i in range(V)]
    movable = [d[i] > 0 and not (pin_boundary and bnd[i]) for i in range(V)]
    for w in weights:
        w = float(np.float32(w))
        new = [row[:] for row in q]
        for i in range(V):
            if not movable[i]:
                continue
            for k in range(3):
                S = 0
                for f in faces:
                    for p in range(3):
                        if f[p] == i:
                            S += q[f[(p + 1) % 3]][k] + q[f[(p + 2) % 3]][k]
                D = S - 2 * d[i] * q[i][k]
                step = int(np.rint((w * float(D)) / float(2 * d[i])))
                new[i][k] = min(max(q[i][k] + step, -2 ** 30), 2 ** 31 - 1)
        q = new
    out = verts.copy()
    for i in range(V):
        if movable[i] and len(weights):
            out[i] = [np.float32(o[k] + float(q[i][k]) * u) for k in range(3)]
    return out, d, bnd


@pytest.mark.parametrize("name", sorted(HAND_MADE))
@pytest.mark.parametrize("pin", [True, False])
def test_reference_equals_the_loop_transcription(name, pin):
    v, f = HAND_MADE[name]()
    for weights in ([], [0.5], [0.5, -0.53] * 3, [-1.0, 1.0, 0.25]):
        want, d, bnd = loop_smooth(v, f, weights, pin_boundary=pin, **UNIT)
        got = M.smooth(v, f, weights, pin_boundary=pin, **UNIT)
        np.testing.assert_array_equal(got["verts"].view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(got["valence"], d)
        np.testing.assert_array_equal(got["boundary"], bnd)


def test_ties_round_to_even_both_ways():
    v, f = one_triangle()
    got = M.smooth(v, f, [0.5], pin_boundary=False, **UNIT)
    assert got["verts"][:, 0].tolist() == [10.0, 11.0, 10.0]     # 0.5 -> 0, -1, 0.5 -> 0
    assert got["verts"][:, 1].tolist() == [12.0, 12.0, 12.0]     # 1.5 -> 2, -1.5 -> -2, 0
    neg = M.smooth(v, f, [-0.5], pin_boundary=False, **UNIT)
    assert neg["verts"][:, 0].tolist() == [10.0, 13.0, 10.0]     # -0.5 -> -0, 1, -0.5 -> -0
    assert neg["verts"][:, 1].tolist() == [8.0, 16.0, 12.0]      # -1.5 -> -2, 1.5 -> 2, 0
    pinned = M.smooth(v, f, [0.5], pin_boundary=True, **UNIT)
    np.testing.assert_array_equal(pinned["verts"], v)
    assert pinned["boundary"].all() and not pinned["movable"].any()


def test_hand_made_valence_and_boundary():
    v, f = repeated_corner()
    assert M.valence(f, len(v)).tolist() == [2, 3, 3, 2, 2, 0]
    # {1,3} twice ([1,1,3]), {2,4} twice ([4,2,4]), {0,2} twice (faces 0 and 3): not boundary
    assert M.boundary(f, len(v)).tolist() == [True, True, True, True, False, False]
    v, f = tetrahedron()
    assert not M.boundary(f, 4).any() and M.valence(f, 4).tolist() == [3, 3, 3, 3]
    v, f = two_triangles()
    assert M.boundary(f, 4).all() and M.valence(f, 4).tolist() == [2, 1, 2, 1]
    # three fins on the edge {0, 1} (multiplicity 3: no boundary by itself), the outer edges
    # once; then every fin twice, and the outer corners 2, 3, 4 joined into a closed strip
    f = np.int64([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 2, 3], [0, 3, 4], [0, 4, 2]])
    assert M.boundary(f[:3], 5).all()
    # {0,1} x3, {1,k} x1, {0,k} x3, {2,3} {3,4} {4,2} x1: vertex 0 has no pair of multiplicity 1
    assert M.boundary(f, 5).tolist() == [False, True, True, True, True]


def test_lattice_of_a_box():
    rng = np.random.default_rng(0)
    for _ in range(50):
        lo = (rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        hi = (lo + rng.random(3) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        if not (hi > lo).any():
            continue
        origin, ul = M.lattice(lo, hi)
        np.testing.assert_array_equal(origin, lo)
        extent = float((hi.astype(np.float64) - lo.astype(np.float64)).max())
        assert 2.0 ** 29 <= extent / 2.0 ** ul <= 2.0 ** 30
        assert (M.quantise(np.stack([lo, hi]), origin, ul) <= 2 ** 30).all()
    assert M.lattice((0, 0, 0), (512, 512, 512))[1] == -20
    assert M.lattice((0, 0, 0), (513, 2, 2))[1] == -20
    assert M.lattice((1.5, 2, 3), (1.5, 2, 3))[1] == M.lattice((0, 0, 0), (1, 1, 1))[1] == -29
    assert math.frexp(1.0) == (0.5, 1)


def test_errors_of_the_definition():
    v, f = two_triangles()
    with pytest.raises(ValueError, match="outside the lattice"):
        M.smooth(v, f, [0.5], (1.0, 0.0, 0.0), 0)
    with pytest.raises(ValueError, match="outside the lattice"):
        M.smooth(v, f, [0.5], (0.0, 0.0, 0.0), -28)
    w = v.copy()
    w[1, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        M.smooth(w, f, [0.5], **UNIT)
    with pytest.raises(ValueError, match=r"outside \[0, V\)"):
        M.smooth(v, [[0, 1, 4]], [0.5], **UNIT)


# --------------------------------------------------------------- properties on the sphere
def _radial(v):
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    return r.mean(), r.std()


def test_taubin_removes_noise_without_shrinking_and_laplacian_shrinks():
    v, f = M.noisy_sphere(5, 0.02)
    assert (len(v), len(f)) == (4098, 8192)
    assert not M.boundary(f, len(v)).any()
    origin, ul = M.lattice(v.min(0), v.max(0))
    _, std0 = _radial(v)
    assert 0.019 < std0 < 0.021
    t = M.smooth(v, f, M.schedule(10, 0.5, -0.53), origin, ul)
    mean_t, std_t = _radial(t["verts"])
    lap = M.smooth(v, f, M.schedule(10, 0.5, None), origin, ul)
    mean_l, std_l = _radial(lap["verts"])
    print(f"input std {std0:.5f}; Taubin std {std_t:.5f} mean {mean_t:.5f}; "
          f"Laplacian std {std_l:.5f} mean {mean_l:.5f}")
    assert std_t < 0.5 * std0 and abs(mean_t - 1.0) < 0.002
    assert mean_l < 0.995 and std_l < std_t
    assert t["movable"].all() and len(M.schedule(10, 0.5, -0.53)) == 20
    # 0 passes: the input's bits
    np.testing.assert_array_equal(M.smooth(v, f, [], origin, ul)["verts"].view(np.uint32),
                                  v.view(np.uint32))


# ----------------------------------------------------------------- properties on the patch
def test_patch_boundary_is_pinned_or_moves():
    v, f = M.patch(20)
    assert (len(v), len(f)) == (400, 2 * 19 * 19)
    origin, ul = M.lattice(v.min(0), v.max(0))
    bnd = M.boundary(f, len(v))
    assert int(bnd.sum()) == 4 * 20 - 4
    ij = np.arange(400).reshape(20, 20)
    border = np.zeros((20, 20), bool)
    border[0] = border[-1] = border[:, 0] = border[:, -1] = True
    np.testing.assert_array_equal(bnd, border.ravel())
    w = M.schedule(5, 0.5, -0.53)
    pinned = M.smooth(v, f, w, origin, ul, pin_boundary=True)
    np.testing.assert_array_equal(pinned["verts"][bnd].view(np.uint32), v[bnd].view(np.uint32))
    assert (pinned["verts"][~bnd] != v[~bnd]).any(1).all()
    assert np.abs(pinned["verts"][~bnd, 2]).std() < np.abs(v[~bnd, 2]).std()
    free = M.smooth(v, f, w, origin, ul, pin_boundary=False)
    assert (free["verts"][bnd] != v[bnd]).any(1).all()
    assert ij[border].size == 76

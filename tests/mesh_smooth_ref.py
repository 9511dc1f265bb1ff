"""NumPy definition of mesh smoothing (include/sdfr.h, "Mesh smoothing"): what
csrc/mesh_smooth.hip is held to.  Test infrastructure; the product never falls back to it.

  lattice(lo, hi)           (origin [3] float32, unit_log2): the default lattice of a box
  quantise(verts, origin, unit_log2)
                            q [V, 3] int64 = rint(((double)v - (double)o) / u); ValueError for
                            a non-finite coordinate or a q outside [0, 2^30]
  valence(faces, V)         d [V] int64: face corners per vertex
  boundary(faces, V)        [V] bool: an end of an edge slot pair of multiplicity exactly 1
  smooth(verts, faces, weights, origin, unit_log2, pin_boundary=True)
                            dict(verts, valence, boundary, movable, q): the passes of
                            ``weights`` in order
  schedule(iterations, lam, mu)
                            the weights of Laplacian (mu None or 0) / Taubin smoothing

Also the meshes the tests share: the subdivided octahedron and the height-field patch.
"""
import math

import numpy as np

Q_MAX = 2 ** 30
CLAMP = (-2 ** 30, 2 ** 31 - 1)
UNIT_LOG2 = (-126, 96)


def lattice(lo, hi):
    lo = np.asarray(lo, np.float32)
    extent = float((np.asarray(hi, np.float64) - lo.astype(np.float64)).max())
    if not extent > 0:
        extent = 1.0
    return lo, math.frexp(extent)[1] - 30


def quantise(verts, origin, unit_log2):
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    assert UNIT_LOG2[0] <= unit_log2 <= UNIT_LOG2[1]
    if not np.isfinite(verts).all():
        raise ValueError("a vertex coordinate is not finite")
    u = 2.0 ** unit_log2
    t = np.rint((verts.astype(np.float64) - np.asarray(origin, np.float32).astype(np.float64)) / u)
    if (t < 0).any() or (t > Q_MAX).any():
        raise ValueError("a vertex is outside the lattice")
    return t.astype(np.int64)


def _faces(faces, V):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("a face index is outside [0, V)")
    return faces


def valence(faces, V):
    return np.bincount(_faces(faces, V).ravel(), minlength=V).astype(np.int64)


def boundary(faces, V):
    faces = _faces(faces, V)
    a = faces.ravel()
    b = faces[:, [1, 2, 0]].ravel()
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    keys, count = np.unique(lo * (1 << 32) + hi, return_counts=True)
    once = keys[count == 1]
    out = np.zeros(V, bool)
    out[once >> 32] = True
    out[once & 0xffffffff] = True
    return out


def one_pass(q, faces, d, movable, w):
    """q [V, 3] int64 -> the next state; ``w`` is the fp32 weight."""
    V = len(q)
    w = float(np.float32(w))
    S = np.zeros((V, 3), np.int64)
    for k in range(3):
        a, b = faces[:, (k + 1) % 3], faces[:, (k + 2) % 3]
        np.add.at(S, faces[:, k], q[a] + q[b])
    m = np.flatnonzero(movable)
    D = S[m] - 2 * d[m, None] * q[m]
    step = np.rint((w * D.astype(np.float64)) / (2 * d[m, None]).astype(np.float64))
    out = q.copy()
    out[m] = np.clip(q[m] + step.astype(np.int64), *CLAMP)
    return out


def smooth(verts, faces, weights, origin, unit_log2, pin_boundary=True):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    V = len(verts)
    faces = _faces(faces, V)
    origin = np.asarray(origin, np.float32)
    q = quantise(verts, origin, unit_log2)
    d = valence(faces, V)
    bnd = boundary(faces, V)
    movable = (d > 0) & ~(bnd & bool(pin_boundary))
    weights = np.asarray(weights, np.float32).reshape(-1)
    assert np.isfinite(weights).all() and (np.abs(weights) <= 1).all() and len(weights) <= 1024
    for w in weights:
        q = one_pass(q, faces, d, movable, w)
    out = verts.copy()
    if len(weights):
        p = origin.astype(np.float64) + q.astype(np.float64) * 2.0 ** unit_log2
        out[movable] = p.astype(np.float32)[movable]
    return dict(verts=out, valence=d, boundary=bnd, movable=movable, q=q)


def schedule(iterations, lam=0.5, mu=-0.53):
    one = [lam] if mu is None or mu == 0 else [lam, mu]
    return np.asarray(one * iterations, np.float32)


# --------------------------------------------------------------------------- shared meshes
NONE = np.zeros((0, 3), np.int64)
# the lattice of the hand-made meshes: integer coordinates are their own q
UNIT = dict(origin=(0.0, 0.0, 0.0), unit_log2=0)


def one_triangle():
    """d = 1 everywhere.  x: D = 2, -4, 2 (w = 0.5: steps 0.5 -> 0, -1, 0.5 -> 0); y: D = 6,
    -6, 0 (steps 1.5 -> 2, -1.5 -> -2, 0)."""
    return np.float32([[10, 10, 5], [12, 14, 5], [10, 12, 5]]), np.int64([[0, 1, 2]])


def tetrahedron():
    v = np.float32([[0, 0, 0], [9, 0, 1], [0, 7, 2], [3, 3, 11]])
    return v, np.int64([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def two_triangles():
    v = np.float32([[0, 0, 0], [8, 0, 3], [8, 8, 0], [0, 9, 5]])
    return v, np.int64([[0, 1, 2], [0, 2, 3]])


def repeated_corner():
    """Face 1 lists vertex 1 twice, face 2 is [i, j, i]; vertex 5 is unreferenced."""
    v = np.float32([[0, 0, 0], [8, 1, 3], [7, 8, 0], [1, 9, 5], [4, 4, 9], [20, 20, 20]])
    return v, np.int64([[0, 1, 2], [1, 1, 3], [4, 2, 4], [0, 2, 3]])


HAND_MADE = {"triangle": one_triangle, "tetrahedron": tetrahedron, "two": two_triangles,
             "repeated": repeated_corner,
             "no_faces": lambda: (np.float32([[1, 2, 3], [4, 5, 6]]), NONE),
             "one_vertex": lambda: (np.float32([[3, 1, 2]]), np.int64([[0, 0, 0]]))}


def octahedron(level=5):
    """A ``level`` times subdivided octahedron on the unit sphere, closed: 4^level * 4 + 2
    vertices, 8 * 4^level faces (float64 vertices)."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.asarray(p, np.float64) for p in v]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        g = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = g
    return np.asarray(v, np.float64), np.asarray(f, np.int64)


def noisy_sphere(level=5, sigma=0.02, seed=0):
    """The octahedron with radial noise of standard deviation ``sigma``: float32 vertices."""
    v, f = octahedron(level)
    r = 1.0 + sigma * np.random.default_rng(seed).standard_normal(len(v))
    return (v * r[:, None]).astype(np.float32), f


def patch(n=20, sigma=0.05, seed=1):
    """An n x n height-field patch (n^2 vertices, 2 (n - 1)^2 faces, 4 n - 4 on the border)
    with noisy z."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = sigma * np.random.default_rng(seed).standard_normal((n, n))
    v = np.stack([i / (n - 1.0), j / (n - 1.0), z], -1).reshape(-1, 3).astype(np.float32)
    c = (i * n + j)[:-1, :-1].ravel()
    f = np.concatenate([np.stack([c, c + n, c + 1], 1), np.stack([c + 1, c + n, c + n + 1], 1)])
    return v, f.astype(np.int64)

"""NumPy definition of mesh connected components (include/sdfr.h, "Mesh connected
components"): what csrc/mesh_cc.hip is held to.  Test infrastructure; the product never
falls back to it.

  labels(faces, V)          label [V]: the smallest vertex index of every vertex's component
                            (min-label propagation over the face edges with pointer jumping)
  dense_ids(label)          (comp [V], C): ids 0..C-1 in increasing order of the smallest vertex
  stats(verts, faces, comp, C)
                            n_vertices, n_faces [C] int64; bbox [C, 6] float32 (min x y z, max
                            x y z over the component's vertices, by the order-preserving
                            uint32 image of the floats); area [C] float64
  select(verts, faces, comp, keep, drop_unreferenced=True)
                            (verts', faces', index_map): order-preserving compaction
  components(verts, faces)  all of it as a dict

Also the meshes the tests share: strip, fan, the two tetrahedra, the two-body volume.
"""
import numpy as np


def labels(faces, V):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    label = np.arange(V, dtype=np.int64)
    if len(faces) == 0:
        return label
    assert faces.min() >= 0 and faces.max() < V
    e0 = np.concatenate([faces[:, 0], faces[:, 1]])
    e1 = np.concatenate([faces[:, 1], faces[:, 2]])
    while True:
        m = np.minimum(label[e0], label[e1])
        new = label.copy()
        np.minimum.at(new, e0, m)
        np.minimum.at(new, e1, m)
        while True:                      # pointer jumping: my label's label, until stable
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, label):
            return label
        label = new


def dense_ids(label):
    label = np.asarray(label, np.int64)
    roots = np.flatnonzero(label == np.arange(len(label)))
    return np.searchsorted(roots, label).astype(np.int64), len(roots)


def float_key(x):
    """Order-preserving uint32 image of float32 (-0 < +0)."""
    u = np.asarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_float(k):
    k = np.asarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return u.view(np.float32)


def face_areas(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((n * n).sum(-1))


def stats(verts, faces, comp, C):
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    comp = np.asarray(comp, np.int64)
    n_vertices = np.bincount(comp, minlength=C).astype(np.int64)
    fc = comp[faces[:, 0]]
    n_faces = np.bincount(fc, minlength=C).astype(np.int64)
    key = float_key(verts)
    lo = np.full((C, 3), 0xffffffff, np.uint32)
    hi = np.zeros((C, 3), np.uint32)
    np.minimum.at(lo, comp, key)
    np.maximum.at(hi, comp, key)
    bbox = np.concatenate([key_float(lo), key_float(hi)], 1)
    area = np.bincount(fc, weights=face_areas(verts, faces), minlength=C).astype(np.float64)
    return n_vertices, n_faces, bbox, area


def components(verts, faces):
    verts = np.asarray(verts, np.float32)
    label = labels(faces, len(verts))
    comp, C = dense_ids(label)
    n_vertices, n_faces, bbox, area = stats(verts, faces, comp, C)
    return dict(label=label, comp=comp, count=C, n_vertices=n_vertices, n_faces=n_faces,
                bbox=bbox, area=area)


def select(verts, faces, comp, keep, drop_unreferenced=True):
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    comp = np.asarray(comp, np.int64)
    keep = np.asarray(keep, bool)
    fkeep = keep[comp[faces[:, 0]]]
    vkeep = keep[comp]
    if drop_unreferenced:
        ref = np.zeros(len(verts), bool)
        ref[faces[fkeep].ravel()] = True
        vkeep = vkeep & ref
    index_map = np.flatnonzero(vkeep)
    new = np.full(len(verts), -1, np.int64)
    new[index_map] = np.arange(len(index_map))
    out_f = new[faces[fkeep]]
    assert (out_f >= 0).all()
    return verts[index_map], out_f, index_map


def largest_mask(size, k):
    """The k largest entries, ties to the lower id."""
    size = np.asarray(size)
    order = np.argsort(-size.astype(np.float64), kind="stable")
    mask = np.zeros(len(size), bool)
    mask[order[:k]] = True
    return mask


# --------------------------------------------------------------------------- shared meshes
def positions(V, seed=0):
    """Some fp32 vertex positions [V, 3] (fixed seed), for meshes given by connectivity."""
    return np.random.default_rng(seed).standard_normal((V, 3)).astype(np.float32)


def two_tetrahedra():
    """Tetrahedron A on the even vertices 0 2 4 6, B on the odd ones 1 3 5 7."""
    t = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    faces = np.empty((8, 3), np.int64)
    faces[0::2] = 2 * t                 # interleaved face rows as well
    faces[1::2] = 2 * t + 1
    return positions(8, 1), faces


def disjoint_triangles(n=1000, loose=37):
    """n triangles on 3 n vertices, then ``loose`` unreferenced vertices."""
    return positions(3 * n + loose, 2), np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def strip(n=4096):
    """A strip of n triangles (i, i + 1, i + 2) on n + 2 vertices."""
    i = np.arange(n, dtype=np.int64)
    return positions(n + 2, 3), np.stack([i, i + 1, i + 2], 1)


def renumber(verts, faces, perm):
    """Vertex i becomes vertex perm[i]."""
    perm = np.asarray(perm, np.int64)
    v = np.empty_like(verts)
    v[perm] = verts
    return v, perm[np.asarray(faces, np.int64)]


def bit_reversed(V):
    """The numbers 0..V-1 ordered by their bit-reversed value: a permutation for any V."""
    bits = max(int(V - 1).bit_length(), 1)
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(V)], np.int64)
    perm = np.empty(V, np.int64)
    perm[np.argsort(rev, kind="stable")] = np.arange(V)
    return perm


def strip_renumberings(n=4096):
    v, f = strip(n)
    V = len(v)
    return {
        "reverse": renumber(v, f, np.arange(V)[::-1]),
        "random": renumber(v, f, np.random.default_rng(7).permutation(V)),
        "bitrev": renumber(v, f, bit_reversed(V)),
    }


def fan(n=8192):
    """n triangles (hub, i, i + 1) around the hub, which has the LARGEST index: V = n + 2."""
    i = np.arange(n, dtype=np.int64)
    hub = n + 1
    return positions(n + 2, 4), np.stack([np.full(n, hub), i, i + 1], 1)


BALL_CENTRE, BALL_RADIUS, SPHERE_RADIUS = (0.8, 0.8, 0.8), 0.1, 0.6


def two_body(points, ball_only=False):
    """The analytic two-body SDF at ``points`` [..., 3] float32: the sphere of radius 0.6 about
    the origin and the ball of radius 0.1 about (0.8, 0.8, 0.8), disjoint; the minimum of the
    two distances, so near the ball the values are the ball-only volume's, bit for bit."""
    d = points - np.asarray(BALL_CENTRE, points.dtype)
    ball = np.sqrt((d * d).sum(-1)) - np.asarray(BALL_RADIUS, points.dtype)
    if ball_only:
        return ball
    return np.minimum(np.sqrt((points * points).sum(-1)) - np.asarray(SPHERE_RADIUS, points.dtype),
                      ball)


def grid_points(res):
    """[res, res, res, 3] float32: c(i) = 2 i / res - 1 per axis, index (ix, iy, iz)."""
    c = (np.arange(res, dtype=np.float32) * np.float32(2) / np.float32(res) - np.float32(1))
    return np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).astype(np.float32)

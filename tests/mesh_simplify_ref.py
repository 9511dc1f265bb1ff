"""NumPy definition of mesh simplification by vertex clustering (include/sdfr.h, "Mesh
simplification"): what csrc/mesh_simplify.hip is held to.  Test infrastructure; the product
never falls back to it.

  cells(verts, origin, cell, dims)     (c [V, 3] int64, q [V, 3] int64, key [V] int64): the cell
                                       of every vertex, its quantised offset inside the cell
                                       (20 fractional bits) and the 64-bit cell key
  simplify(verts, faces, origin, cell, dims, drop_unreferenced=True)
                                       dict: verts, faces, index_map, cluster, members, plus
                                       count (C), nondegenerate (faces with three distinct
                                       clusters, before the duplicates go)

fp32 steps in np.float32 (one rounded operation each), the position in np.float64, the
duplicate classes by a dict over the sorted cluster triples.
"""
import numpy as np


def cells(verts, origin, cell, dims):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    o = np.asarray(origin, np.float32)
    h = np.float32(cell)
    n = np.asarray(dims, np.int64)
    assert np.isfinite(v).all() and np.isfinite(o).all() and np.isfinite(h) and h > 0
    assert n.shape == (3,) and (n >= 1).all() and (n <= 2 ** 21).all()
    with np.errstate(over="ignore"):
        t = (v - o) / h                                        # two rounded fp32 operations
    assert t.dtype == np.float32
    cf = np.clip(np.floor(t), np.float32(0), (n - 1).astype(np.float32))   # clamped as float
    with np.errstate(invalid="ignore"):
        r = np.clip(t - cf, np.float32(0), np.float32(1))
    assert cf.dtype == np.float32 and r.dtype == np.float32
    c = cf.astype(np.int64)
    q = np.rint(r.astype(np.float64) * 2.0 ** 20).astype(np.int64)   # exact product, half-even
    key = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    return c, q, key


def simplify(verts, faces, origin, cell, dims, drop_unreferenced=True):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    assert V >= 1 and (len(f) == 0 or (f.min() >= 0 and f.max() < V))
    c, q, key = cells(v, origin, cell, dims)
    # rep = the smallest vertex index of the cell; clusters in increasing order of rep
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rep = first[inv.reshape(-1)]
    reps = np.flatnonzero(rep == np.arange(V))
    pre = np.searchsorted(reps, rep)                           # cluster id before the drop
    C = len(reps)
    m = np.bincount(pre, minlength=C).astype(np.int64)
    S = np.zeros((C, 3), np.int64)
    np.add.at(S, pre, q)
    o64 = np.asarray(origin, np.float32).astype(np.float64)
    mean = S.astype(np.float64) / (m.astype(np.float64) * 2.0 ** 20)[:, None]
    pos = (o64 + (c[reps].astype(np.float64) + mean) * np.float64(np.float32(cell))).astype(
        np.float32)
    g = pre[f]
    ok = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    s = np.sort(g, 1)
    seen = set()
    keepf = np.zeros(len(f), bool)
    for i in np.flatnonzero(ok):                               # increasing face index
        k = (int(s[i, 0]), int(s[i, 1]), int(s[i, 2]))
        if k not in seen:
            seen.add(k)
            keepf[i] = True
    used = np.ones(C, bool)
    if drop_unreferenced:
        used = np.zeros(C, bool)
        used[g[keepf].ravel()] = True
    new = np.cumsum(used) - 1
    return dict(verts=pos[used], faces=new[g[keepf]].reshape(-1, 3), index_map=reps[used],
                cluster=np.where(used[pre], new[pre], -1), members=m[used], count=C,
                nondegenerate=int(ok.sum()))


def vertex_sets(faces):
    """The faces as sorted rows, for the duplicate and degeneracy properties."""
    return np.sort(np.asarray(faces, np.int64).reshape(-1, 3), 1)

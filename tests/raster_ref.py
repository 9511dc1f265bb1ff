"""References for the mesh rasteriser (include/sdfr.h, "Mesh rasteriser").

``raster_ref`` / ``interp_ref``: the definition transcribed op for op in NumPy float32 and
int64 -- every product, sum and quotient is one rounded fp32 operation, every integer step
exact -- so the HIP kernels must reproduce it bit for bit.  It visits every pixel for every
triangle: no bounding boxes, no small / large split.

``raycast_ref``: an independent float64 formulation with no projection in it:
Moeller-Trumbore intersection of the render's own rays with every triangle, nearest hit.

``icosphere``, ``look_at``: test geometry.
"""
import math

import numpy as np

f32 = np.float32
SUB = 4096            # 12 subpixel bits
HALF = SUB // 2

# The comparison's inputs (tests/test_raster.py): the icosphere with 2 subdivisions, radius
# 0.1, at the origin; look-at cameras at distance 1, (azimuth, elevation, resolution), focal
# (res / 2) / tan(6 degrees).
VIEWS = ((0.3, 0.15, 32), (-0.4, 0.0, 32), (0.0, 0.0, 48))
# Measured on those inputs with the two references below (depth near 1): raster_ref's fp32
# depth differs from the float64 ray cast's by at most 9.81e-6 (per view 9.81e-6, 5.18e-6,
# 4.86e-6).  The bound is 3x the measured maximum.
DEPTH_BOUND = 3 * 9.81e-6
# Same inputs: the fp32 interpolated position lies within 7.28e-7 (max over x, y, z; per view
# 7.28e-7, 7.13e-7, 4.49e-7) of the float64 point o + d * depth on the pixel's ray.  3x.
RAY_BOUND = 3 * 7.28e-7


def icosphere(subdivisions=2, radius=1.0):
    """(vertices [V,3] float32, faces [F,3] int64), counter-clockwise about the outward
    normal: 12 / 20 at 0 subdivisions, 42 / 80, 162 / 320, ..."""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p),
         (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4),
         (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
         (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, np.int64)


def look_at(azim, elev, dist=1.0):
    """Camera-to-world [3,4] float32 of a camera at ``dist`` from the origin at azimuth /
    elevation (radians), looking at the origin, y up; the camera looks along its -z."""
    pos = dist * np.array([math.cos(elev) * math.sin(azim), math.sin(elev),
                           math.cos(elev) * math.cos(azim)])
    z = pos / np.linalg.norm(pos)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), pos[:, None]], 1).astype(np.float32)


def fov_focal(res, half_angle_deg=6.0):
    return (res / 2) / math.tan(math.radians(half_angle_deg))


def project_ref(vertices, cam, focal, cx, cy, znear):
    """One view: (X, Y int64, z, rz float32, usable bool), each [V]."""
    v = np.asarray(vertices, f32)
    cam = np.asarray(cam, f32)
    focal, cx, cy, znear = f32(focal), f32(cx), f32(cy), f32(znear)
    with np.errstate(all="ignore"):
        d = [v[:, m] - cam[m, 3] for m in range(3)]
        q = [(d[0] * cam[0, k] + d[1] * cam[1, k]) + d[2] * cam[2, k] for k in range(3)]
        z = -q[2]
        x = cx + (focal * q[0]) / z
        y = cy - (focal * q[1]) / z
        xs, ys = np.rint(x * f32(SUB)), np.rint(y * f32(SUB))
        ok = np.isfinite(z) & (z > znear) & (np.abs(xs) < f32(2 ** 30)) & (np.abs(ys) < f32(2 ** 30))
        X = np.where(ok, xs, 0).astype(np.int64)
        Y = np.where(ok, ys, 0).astype(np.int64)
        rz = f32(1) / z
    for a in (z, x, y, xs, rz):
        assert a.dtype == np.float32
    return X, Y, z, rz, ok


def raster_ref(vertices, faces, cam, focal, H, W, znear=0.01):
    """``(face_idx [B,H,W] int32, depth [B,H,W] float32, bary [B,H,W,3] float32)``."""
    faces = np.asarray(faces, np.int64)
    cam = np.asarray(cam, f32)
    B, V = cam.shape[0], len(vertices)
    focal = np.broadcast_to(np.asarray(focal, f32).reshape(-1), (B,))
    Px = (np.arange(W, dtype=np.int64) * SUB + HALF)[None, :]
    Py = (np.arange(H, dtype=np.int64) * SUB + HALF)[:, None]
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    face_idx = np.full((B, H, W), -1, np.int32)
    depth = np.zeros((B, H, W), f32)
    bary = np.zeros((B, H, W, 3), f32)
    for b in range(B):
        X, Y, _, rz, ok = project_ref(vertices, cam[b], focal[b], W / 2, H / 2, znear)
        keys = np.full((H, W), empty, np.uint64)
        for fid, (a, bb, c) in enumerate(faces):
            if min(a, bb, c) < 0 or max(a, bb, c) >= V or not (ok[a] and ok[bb] and ok[c]):
                continue
            A = (X[bb] - X[a]) * (Y[c] - Y[a]) - (Y[bb] - Y[a]) * (X[c] - X[a])
            if A == 0:
                continue
            w1 = (Px - X[a]) * (Y[c] - Y[a]) - (Py - Y[a]) * (X[c] - X[a])
            w2 = (X[bb] - X[a]) * (Py - Y[a]) - (Y[bb] - Y[a]) * (Px - X[a])
            w0 = A - w1 - w2
            if A < 0:
                w0, w1, w2 = -w0, -w1, -w2
            cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
            if not cov.any():
                continue
            fA = np.abs(np.asarray(A, np.int64)).astype(f32)          # int64 -> fp32, one rounding
            with np.errstate(all="ignore"):
                l0, l1, l2 = w0.astype(f32) / fA, w1.astype(f32) / fA, w2.astype(f32) / fA
                iz = (l0 * rz[a] + l1 * rz[bb]) + l2 * rz[c]
                dep = f32(1) / iz
                bar = np.stack([(l0 * rz[a]) * dep, (l1 * rz[bb]) * dep, (l2 * rz[c]) * dep], -1)
            assert dep.dtype == np.float32 and bar.dtype == np.float32
            cov &= (dep > 0) & np.isfinite(dep)
            key = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(fid)
            win = cov & (key < keys)
            keys[win] = key[win]
            face_idx[b][win] = fid
            depth[b][win] = dep[win]
            bary[b][win] = bar[win]
    return face_idx, depth, bary


def interp_ref(attr, faces, face_idx, bary, background=None, fill=0.0):
    """``interpolate_vertex_attributes`` in NumPy float32: [B,C,H,W]."""
    attr = np.asarray(attr, f32)
    if attr.ndim == 1:
        attr = attr[:, None]
    faces = np.asarray(faces, np.int64)
    B, H, W = face_idx.shape
    C = attr.shape[1]
    cov = face_idx >= 0
    tri = faces[np.where(cov, face_idx, 0)]                              # [B,H,W,3]
    a0, a1, a2 = (attr[tri[..., k]] for k in range(3))                   # [B,H,W,C]
    val = (bary[..., 0:1] * a0 + bary[..., 1:2] * a1) + bary[..., 2:3] * a2
    assert val.dtype == np.float32
    val = np.moveaxis(val, -1, 1)
    if background is not None:
        bg = np.broadcast_to(np.asarray(background, f32), (B, C, H, W))
    else:
        bg = np.full((B, C, H, W), f32(fill), f32)
    return np.where(cov[:, None], val, bg).astype(f32)


def rays_ref(cam, focal, H, W):
    """The render's rays in float64: origin [3], directions [H,W,3] (unnormalised, camera
    z = -1) of pixel centres (i + 0.5, j + 0.5), principal point (W/2, H/2)."""
    cam = np.asarray(cam, np.float64)
    i = np.arange(W, dtype=np.float64) + 0.5
    j = np.arange(H, dtype=np.float64) + 0.5
    dx = np.broadcast_to(((i - W / 2) / focal)[None, :], (H, W))
    dy = np.broadcast_to((-(j - H / 2) / focal)[:, None], (H, W))
    dirs = np.stack([dx, dy, -np.ones((H, W))], -1)
    return cam[:, 3], dirs @ cam[:, :3].T


def raycast_ref(vertices, faces, cam, focal, H, W):
    """One view in float64: ``(face_idx [H,W] (-1: miss), t [H,W] the ray parameter = camera
    depth, bary [H,W,3])`` of the nearest Moeller-Trumbore hit."""
    v = np.asarray(vertices, np.float64)
    faces = np.asarray(faces, np.int64)
    o, d = rays_ref(np.asarray(cam, f32), float(f32(focal)), H, W)
    d = d.reshape(-1, 1, 3)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = (v1 - v0)[None], (v2 - v0)[None]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tv = (o - v0)[None]
        u = (tv * pv).sum(-1) * inv
        qv = np.cross(tv, e1)
        w = (d * qv).sum(-1) * inv
        t = (e2 * qv).sum(-1) * inv
    hit = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
    t = np.where(hit, t, np.inf)
    best = t.argmin(1)
    rows = np.arange(t.shape[0])
    tb = t[rows, best]
    any_hit = np.isfinite(tb)
    fid = np.where(any_hit, best, -1).reshape(H, W)
    ub, wb = u[rows, best], w[rows, best]
    bar = np.stack([1 - ub - wb, ub, wb], -1)
    bar = np.where(any_hit[:, None], bar, 0.0).reshape(H, W, 3)
    return fid, np.where(any_hit, tb, 0.0).reshape(H, W), bar

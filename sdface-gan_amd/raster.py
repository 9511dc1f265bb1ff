"""Looking at a mesh: the HIP rasteriser (csrc/raster.hip, ``sdfr_mesh_raster`` /
``sdfr_mesh_interpolate``) and what is built on it.

Where the reference hands a marching-cubes mesh to pytorch3d (sdf_utils.py:209-331, and
``NoiseInjection.project_noise``, sdf_model.py:713-792), ``rasterize_mesh`` draws B views of
one ``Mesh`` with the render's own pinhole camera: per pixel the nearest triangle, its camera
depth and perspective-correct barycentrics, deterministic bit for bit (the definition is
pinned in include/sdfr.h, "Mesh rasteriser").  ``interpolate_vertex_attributes`` turns any
per-vertex quantity into an image through that result; ``render_mesh`` returns the
``Surface`` that ``render_surface`` returns, from the mesh instead of the field -- cost
proportional to the triangles, no network needed -- and ``shade_surface`` lights it.
``load_obj`` reads what ``Mesh.export`` writes; ``subdivide_mesh`` is the midpoint
subdivision the reference applies (trimesh.remesh.subdivide) before it rasterises at 256^2
and above.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from .mesh import Mesh

# What rasterize_mesh returns: face_idx [B,H,W] int32 (the triangle's row in ``faces``, -1
# where nothing covers the pixel), depth [B,H,W] (camera depth; 0 uncovered) and bary
# [B,H,W,3] (perspective-correct barycentrics; 0 uncovered).
Raster = namedtuple("Raster", ("face_idx", "depth", "bary"))


def _check_faces(mesh: Mesh):
    """Host range check of ``mesh.faces`` against its vertex count, once per (vertices,
    faces) pair: ValueError for an index outside [0, V)."""
    v, f = mesh.vertices, mesh.faces
    seen = getattr(mesh, "_sdfr_checked", None)
    if seen is not None and seen[0] is v and seen[1] is f:
        return
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"mesh: vertices must be [V, 3] and faces [F, 3], got "
                         f"{v.shape} and {f.shape}")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError(f"mesh: face indices must lie in [0, {v.shape[0]}), got "
                         f"[{int(f.min())}, {int(f.max())}]")
    mesh._sdfr_checked = (v, f)


def _mesh_device(mesh: Mesh, device):
    """``(vertices [V,3] fp32, faces [F,3] int32)`` of ``mesh`` on ``device``: uploaded once
    per (vertices, faces) pair and kept on the mesh."""
    _check_faces(mesh)
    cache = getattr(mesh, "_sdfr_dev", None)
    if cache is None:
        cache = mesh._sdfr_dev = {}
    hit = cache.get(device)
    if hit is None or hit[0] is not mesh.vertices or hit[1] is not mesh.faces:
        v = torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float32)).to(device)
        f = torch.from_numpy(np.ascontiguousarray(mesh.faces).astype(np.int32)).to(device)
        hit = cache[device] = (mesh.vertices, mesh.faces, v, f)
    return hit[2], hit[3]


def _focal_vector(focal, B, device):
    if torch.is_tensor(focal):
        f = focal.detach().to(device=device, dtype=torch.float32).reshape(-1)
        if f.numel() == 1 and B != 1:
            f = f.expand(B)
        if f.numel() != B:
            raise ValueError(f"focal must be a number, [B], or [B,1,1] with B = {B}, got "
                             f"{tuple(focal.shape)}")
        return f.contiguous()
    return torch.full((B,), float(focal), dtype=torch.float32, device=device)


def _hw(res):
    if isinstance(res, (tuple, list)):
        H, W = int(res[0]), int(res[1])
    else:
        H = W = int(res)
    if H < 1 or W < 1:
        raise ValueError(f"res must be positive, got {res}")
    return H, W


def rasterize_mesh(mesh: Mesh, cam_poses, focal, res, znear: float = 0.01) -> Raster:
    """``Raster(face_idx, depth, bary)`` of ``mesh`` seen from the B cameras ``cam_poses``
    [B,3,4] (camera-to-world, as the renderer takes them) at ``res`` (an int, or (H, W)),
    principal point at the image centre.  ``focal`` is [B], [B,1,1] or a number, in pixels of
    that image.  The pixel (row j, column i) is the one whose ray the renderer casts through
    (i + 0.5, j + 0.5); its triangle is the nearest one that covers its centre (the smallest
    row of ``faces`` among equal depths), triangles with a vertex at depth <= ``znear`` are
    dropped whole.  ValueError for a face index outside [0, V) (checked on the host, once
    per mesh); RuntimeError for CPU tensors."""
    from . import _lib
    _check_faces(mesh)
    H, W = _hw(res)
    if not (torch.is_tensor(cam_poses) and cam_poses.is_cuda):
        raise RuntimeError("rasterize_mesh: needs the GPU (HIP kernel)")
    if cam_poses.dim() != 3 or cam_poses.shape[1] < 3 or cam_poses.shape[2] != 4:
        raise ValueError(f"rasterize_mesh: cam_poses must be [B,3,4], got "
                         f"{tuple(cam_poses.shape)}")
    dev = cam_poses.device
    B = cam_poses.shape[0]
    cam = cam_poses.detach()[:, :3, :].to(torch.float32).contiguous()
    foc = _focal_vector(focal, B, dev)
    face_idx = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    depth = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    bary = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    if B == 0 or V == 0 or F == 0:
        return Raster(face_idx.fill_(-1), depth.zero_(), bary.zero_())
    verts, faces = _mesh_device(mesh, dev)
    L = _lib.lib()
    need = L.sdfr_mesh_raster_workspace_bytes(B, H, W, V, F)
    if need == 0:
        raise ValueError("rasterize_mesh: H and W must be <= 16384, and B V, B F and B H W "
                         "below 2^31")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    a = _lib.RasterArgs(B=B, H=H, W=W, V=V, F=F, vertices=_lib.ptr(verts),
                        faces=_lib.ptr(faces), cam=_lib.ptr(cam), focal=_lib.ptr(foc),
                        cx=W / 2, cy=H / 2, znear=float(znear), face_idx=_lib.ptr(face_idx),
                        depth=_lib.ptr(depth), bary=_lib.ptr(bary), workspace=_lib.ptr(ws),
                        workspace_bytes=need)
    _lib.check(L.sdfr_mesh_raster(ctypes.byref(a), _lib.stream_of(cam)), "sdfr_mesh_raster")
    return Raster(face_idx, depth, bary)


def interpolate_vertex_attributes(mesh: Mesh, raster: Raster, attr, background=None,
                                  fill: float = 0.0) -> torch.Tensor:
    """The per-vertex attribute ``attr`` [V, C] (or [V]; array or tensor) as an image
    [B, C, H, W] through ``raster``: at a covered pixel
    ``(bary0 attr[i0] + bary1 attr[i1]) + bary2 attr[i2]`` over its triangle's vertices, at
    an uncovered one ``background`` ([1 or B, C, H, W]) when given, else ``fill``."""
    from . import _lib
    face_idx, bary = raster.face_idx, raster.bary
    if not face_idx.is_cuda:
        raise RuntimeError("interpolate_vertex_attributes: needs the GPU (HIP kernel)")
    dev = face_idx.device
    B, H, W = face_idx.shape
    attr = torch.as_tensor(attr).detach().to(device=dev, dtype=torch.float32)
    if attr.dim() == 1:
        attr = attr[:, None]
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    if attr.dim() != 2 or attr.shape[0] != V or attr.shape[1] < 1:
        raise ValueError(f"interpolate_vertex_attributes: attr must be [V, C] with V = {V}, "
                         f"got {tuple(attr.shape)}")
    attr = attr.contiguous()
    C = attr.shape[1]
    bg_batch = 0
    if background is not None:
        background = background.detach().to(device=dev, dtype=torch.float32).contiguous()
        if background.shape[0] not in (1, B) or tuple(background.shape[1:]) != (C, H, W):
            raise ValueError(f"interpolate_vertex_attributes: background must be "
                             f"[1 or {B}, {C}, {H}, {W}], got {tuple(background.shape)}")
        bg_batch = background.shape[0]
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    if B == 0:
        return out
    if V == 0 or F == 0:
        if background is not None:
            return out.copy_(background.expand(B, C, H, W))
        return out.fill_(fill)
    _, faces = _mesh_device(mesh, dev)
    _lib.check(_lib.lib().sdfr_mesh_interpolate(
        _lib.ptr(attr), V, C, _lib.ptr(faces), F, _lib.ptr(face_idx.contiguous()),
        _lib.ptr(bary.contiguous()), B, H, W, _lib.ptr(background), bg_batch, float(fill),
        _lib.ptr(out), _lib.stream_of(out)), "sdfr_mesh_interpolate")
    return out


MESH_FIELDS = ("hit", "depth", "xyz", "normal", "rgb")


def render_mesh(mesh: Mesh, cam_poses, focal, res, want=MESH_FIELDS, znear: float = 0.01):
    """The mesh as an image: the ``Surface`` of ``render_surface`` (``sample``, ``residual``
    and ``sdf`` are ``None``), so ``shade_surface`` lights it unchanged.  ``hit`` [B,1,H,W]
    is 1.0 where a triangle covers the pixel, ``depth`` [B,1,H,W] the camera depth (what
    ``render_surface``'s is: the ray direction has camera z = -1), ``xyz`` [B,3,H,W] the
    interpolated vertex positions, ``normal`` the interpolated ``vertex_normals`` divided by
    ``max(|.|, 1e-20)`` -- without ``vertex_normals`` the triangle's
    ``(v1 - v0) x (v2 - v0)`` normalised the same way (faces wind counter-clockwise about
    the outward normal) -- and ``rgb`` the interpolated ``vertex_colors`` (``None`` without
    them).  Every float map is 0 where nothing is hit."""
    from .renderer import Surface
    want = tuple(want)
    unknown = [k for k in want if k not in MESH_FIELDS]
    if unknown or not want:
        raise ValueError(f"render_mesh: want must name some of {MESH_FIELDS}, got {want}")
    r = rasterize_mesh(mesh, cam_poses, focal, res, znear)
    out = {}
    hit = (r.face_idx >= 0).unsqueeze(1)
    if "hit" in want:
        out["hit"] = hit.to(torch.float32)
    if "depth" in want:
        out["depth"] = r.depth.unsqueeze(1)
    if "xyz" in want:
        out["xyz"] = interpolate_vertex_attributes(mesh, r, mesh.vertices)
    if "normal" in want:
        if mesh.vertex_normals is not None:
            n = interpolate_vertex_attributes(mesh, r, mesh.vertex_normals)
        else:
            v, f = _mesh_device(mesh, r.face_idx.device)
            n = r.bary.new_zeros(r.face_idx.shape + (3,))
            if f.shape[0]:
                f = f.long()
                v0 = v[f[:, 0]]
                fn = torch.linalg.cross(v[f[:, 1]] - v0, v[f[:, 2]] - v0)
                n = fn[r.face_idx.clamp_min(0).long()] * hit.squeeze(1).unsqueeze(-1)
            n = n.permute(0, 3, 1, 2).contiguous()
        out["normal"] = n / n.norm(dim=1, keepdim=True).clamp_min(1e-20)
    if "rgb" in want and mesh.vertex_colors is not None:
        out["rgb"] = interpolate_vertex_attributes(mesh, r, mesh.vertex_colors)
    return Surface(**{k: out.get(k) for k in Surface._fields})


def load_obj(path_or_file) -> Mesh:
    """The ``Mesh`` of a Wavefront .obj as ``Mesh.export`` writes it: ``v x y z [r g b]``,
    ``vn x y z`` and ``f a b c`` / ``f a//a b//b c//c`` lines (1-based; ``a/t/n`` forms are
    read for their vertex index, negative indices count from the end, polygons become
    fans).  Colours are kept when every vertex has one, normals when there is one per
    vertex; everything else in the file is ignored."""
    if hasattr(path_or_file, "read"):
        text = path_or_file.read()
    else:
        with open(path_or_file) as fh:
            text = fh.read()
    verts, colors, normals, faces = [], [], [], []
    for line in text.splitlines():
        p = line.split()
        if not p:
            continue
        if p[0] == "v":
            verts.append(p[1:4])
            if len(p) >= 7:
                colors.append(p[4:7])
        elif p[0] == "vn":
            normals.append(p[1:4])
        elif p[0] == "f":
            idx = [int(t.split("/")[0]) for t in p[1:]]
            idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
            for k in range(1, len(idx) - 1):
                faces.append((idx[0], idx[k], idx[k + 1]))
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = np.asarray(colors, np.float32).reshape(-1, 3) if len(colors) == len(verts) and verts \
        else None
    n = np.asarray(normals, np.float32).reshape(-1, 3) if len(normals) == len(verts) and verts \
        else None
    return Mesh(v, f, vertex_colors=c, vertex_normals=n)


def _subdivide_once(mesh: Mesh) -> Mesh:
    v = torch.from_numpy(mesh.vertices)
    f = torch.from_numpy(mesh.faces)
    V = v.shape[0]
    if f.shape[0] == 0:
        return mesh
    a, b, c = f.unbind(1)
    ends = torch.stack([torch.stack([a, b], 1), torch.stack([b, c], 1),
                        torch.stack([c, a], 1)], 1)                     # [F, 3 (ab, bc, ca), 2]
    lo, hi = ends.min(-1).values, ends.max(-1).values
    edges, inv = torch.unique((lo * V + hi).reshape(-1), sorted=True, return_inverse=True)
    elo, ehi = edges // V, edges % V
    ab, bc, ca = (V + inv.reshape(-1, 3)).unbind(1)
    faces = torch.stack([torch.stack([a, ab, ca], 1), torch.stack([b, bc, ab], 1),
                         torch.stack([c, ca, bc], 1), torch.stack([ab, bc, ca], 1)],
                        1).reshape(-1, 3)

    def grow(x):
        if x is None:
            return None
        x = torch.from_numpy(x)
        return torch.cat([x, (x[elo] + x[ehi]) * 0.5])

    normals = grow(mesh.vertex_normals)
    if normals is not None:
        new = normals[V:]
        normals[V:] = new / new.norm(dim=1, keepdim=True).clamp_min(1e-20)
        normals = normals.numpy()
    colors = grow(mesh.vertex_colors)
    return Mesh(grow(mesh.vertices).numpy(), faces.numpy(),
                vertex_colors=None if colors is None else colors.numpy(),
                vertex_normals=normals)


def subdivide_mesh(mesh: Mesh, times: int = 1) -> Mesh:
    """Midpoint subdivision, ``times`` times (plain torch on the host; stands in for
    trimesh.remesh.subdivide): every triangle becomes four, every edge gets one new vertex
    at its midpoint, shared by the triangles on both sides.  The new vertices follow the
    old ones in ascending order of their edge (min index, max index); with ab, bc, ca the
    midpoints of face f = (a, b, c), its children are rows 4f .. 4f+3:
    [a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca] (the winding is kept).  Colours and
    normals of a new vertex are the mean of its edge's ends, normals renormalised."""
    _check_faces(mesh)
    for _ in range(int(times)):
        mesh = _subdivide_once(mesh)
    return mesh


def default_projection_focal(res: int) -> float:
    """The focal length in pixels of the reference's projection camera (fov 12 degrees,
    sdf_model.py:762) at ``res`` pixels: (res / 2) / tan(6 degrees)."""
    return (res / 2) / math.tan(math.radians(6.0))

"""Surface extraction of sdf_mesh.py (im2scene/sdf/models/sdf_utils.py:164-223).

The SDF volume itself comes from the fused renderer: sdf_mesh.py builds a second
Generator at 128^2 rays x 128 samples with return_sdf / return_xyz
(sdf_mesh.py:244-252), whose forward runs ``sdfr_render_ngp_forward`` like any
other render and returns the per-sample SDF as a [B, H, W, N, 1] volume.
``align_volume`` resamples that frustum-shaped volume onto a cube (device-side
``grid_sample``, any device).  ``extract_mesh_with_marching_cubes`` runs the
HIP marching cubes (csrc/mesh.hip, ``sdfr_mc_count`` / ``sdfr_mc_emit``) where
the reference calls scikit-image on the host, applies the reference's vertex
scaling and axis flips, and returns a ``Mesh`` whose ``export(f, file_type='obj')``
writes the .obj that sdf_mesh.py:176-182 writes through trimesh.

Beyond the reference, the field can be queried directly (``VolumeFeatureRenderer.query``,
``sdfr_query_ngp_forward``): ``sdf_cube`` evaluates the SDF on the cube marching cubes
reads -- no frustum render, no ``align_volume`` resampling -- and ``color_mesh`` asks the
field for the colour at every vertex (``Mesh.vertex_colors``, written as ``v x y z r g b``).
``normal_mesh`` asks it for the SDF's gradient there (``VolumeFeatureRenderer.query_gradient``,
``sdfr_query_ngp_grad``; ``Mesh.vertex_normals``, written as ``vn x y z``), and
``eikonal_residual`` gives ``|grad sdf| - 1`` in world units at any points.

``extract_mesh_sparse`` is ``sdf_cube`` + ``extract_mesh_with_marching_cubes`` without the
dense cube: the field on the 8^3-point bricks near the surface only, marching cubes on
that storage (csrc/mesh_sparse.hip), growth along the surface into bricks the first guess
missed -- up to 1024^3.  ``sparse_extract`` is the driver for any field, ``SparseVolume``
what it stored.

``mesh_components`` / ``keep_components`` split a mesh into its connected components and keep
the wanted ones on the GPU (csrc/mesh_cc.hip, ``sdfr_mesh_cc_*``): the field's mesh is the
face plus whatever the untrained space outside the camera frustum holds, and
``keep_components(mesh, largest=1)`` -- or ``extract_mesh_sparse(..., components={"largest":
1})``, before the copy to the host -- is what trimesh's ``mesh.split()`` is used for.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F


def align_volume(volume: torch.Tensor, near: float = 0.88, far: float = 1.12) -> torch.Tensor:
    """Frustum -> cube resampling of an SDF volume [1, H, W, D, C] (sdf_utils.py:164).

    The x/y sampling coordinates of depth slice k are scaled by
    linspace(far/near, 1, D)[k]; trilinear grid_sample with border padding and
    align_corners; cube cells whose scaled coordinate leaves [-1, 1] are set to 1
    so marching cubes sees "outside" there.  As in the reference the sampling grid
    has batch 1, so only single-volume batches are accepted (grid_sample raises
    otherwise).
    """
    b, h, w, d, c = volume.shape
    dev = volume.device
    # the 1-D linspaces come from the CPU (the reference's values, bit for bit);
    # the h*w*d grid is formed on the volume's device -- built on the host it
    # was a 200 MB copy per 256^3 volume (52 ms)
    lin = [torch.linspace(-1, 1, n).to(dev) for n in (h, w, d)]
    yy, xx, zz = torch.meshgrid(lin[0], lin[1], lin[2], indexing="ij")
    grid = torch.stack([xx, yy, zz], -1).unsqueeze(0)                     # [1,h,w,d,3]
    scale = torch.linspace(far / near, 1, d).view(1, 1, 1, -1, 1).to(dev)
    grid[..., :2] = grid[..., :2] * scale
    outside = torch.any(grid.lt(-1).logical_or(grid.gt(1)), -1, keepdim=True)
    sampled = F.grid_sample(volume.permute(0, 4, 3, 1, 2).contiguous(),
                            grid.permute(0, 3, 1, 2, 4).contiguous(),
                            padding_mode="border", align_corners=True)
    out = sampled.permute(0, 3, 4, 2, 1).contiguous()
    if out.shape[-1] != 1:
        out[outside] = 1            # the reference's boolean-index path (and its errors)
    else:
        out.masked_fill_(outside, 1.0)   # same cells, no host sync
    return out


class Mesh:
    """Indexed triangle mesh: ``vertices`` [V, 3] float32, ``faces`` [F, 3] int64
    (counter-clockwise about the outward normal).  Stands in for the
    ``trimesh.Trimesh`` the reference returns; trimesh's merge / cleanup
    processing is not applied (vertices are already unique per grid edge);
    ``mesh_components`` / ``keep_components`` stand in for ``split()``."""

    def __init__(self, vertices, faces, vertex_colors=None, vertex_normals=None):
        self.vertices = np.asarray(vertices, np.float32)
        self.faces = np.asarray(faces, np.int64)
        # None, or [V, 3] RGB in [0, 1] (color_mesh)
        self.vertex_colors = (None if vertex_colors is None
                              else np.asarray(vertex_colors, np.float32))
        # None, or [V, 3] unit normals (normal_mesh)
        self.vertex_normals = (None if vertex_normals is None
                               else np.asarray(vertex_normals, np.float32))

    def export(self, file_obj=None, file_type="obj"):
        """Wavefront .obj text (``v x y z`` lines -- ``v x y z r g b`` when
        ``vertex_colors`` is set -- then 1-based ``f a b c``; with ``vertex_normals`` set,
        ``vn x y z`` lines follow the ``v`` lines and faces are ``f a//a b//b c//c``);
        written to ``file_obj`` (an open text file or a path) when given."""
        if file_type != "obj":
            raise ValueError(f"Mesh.export: only 'obj' is supported, not {file_type!r}")
        if self.vertex_colors is None:
            lines = ["v %.8f %.8f %.8f" % tuple(v) for v in self.vertices.tolist()]
        else:
            if self.vertex_colors.shape != self.vertices.shape:
                raise ValueError("Mesh.export: vertex_colors must be [V, 3] like vertices")
            lines = ["v %.8f %.8f %.8f %.6f %.6f %.6f" % tuple(v + c) for v, c in
                     zip(self.vertices.tolist(), self.vertex_colors.tolist())]
        if self.vertex_normals is None:
            lines += ["f %d %d %d" % tuple(f) for f in (self.faces + 1).tolist()]
        else:
            if self.vertex_normals.shape != self.vertices.shape:
                raise ValueError("Mesh.export: vertex_normals must be [V, 3] like vertices")
            lines += ["vn %.6f %.6f %.6f" % tuple(n) for n in self.vertex_normals.tolist()]
            lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c)
                      for a, b, c in (self.faces + 1).tolist()]
        text = "\n".join(lines) + "\n"
        if file_obj is None:
            return text
        if hasattr(file_obj, "write"):
            file_obj.write(text)
        else:
            with open(file_obj, "w") as f:
                f.write(text)
        return text


def marching_cubes(volume: torch.Tensor, level: float = 0.0):
    """Zero (``level``) set of an fp32 volume [n0, n1, n2] on the GPU (any strides):
    (verts [V, 3] fp32 in index coordinates, faces [F, 3] int32), both on the
    volume's device.  ValueError when no grid edge crosses ``level`` (scikit-image
    raises ValueError for a level outside the data range, which sdf_mesh.py:170-174
    catches)."""
    from . import _lib
    if volume.dim() != 3:
        raise ValueError(f"marching_cubes: expected a 3-D volume, got {tuple(volume.shape)}")
    if not volume.is_cuda:
        raise RuntimeError("marching_cubes: the volume must be on the GPU (HIP kernel)")
    if volume.dtype != torch.float32:
        volume = volume.float()
    L = _lib.lib()
    n0, n1, n2 = volume.shape
    s0, s1, s2 = volume.stride()
    ws_bytes = L.sdfr_mc_workspace_bytes(n0, n1, n2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=volume.device)
    counts = (_lib._u32 * 2)()
    st = _lib.stream_of(volume)
    args = (_lib.ptr(volume), n0, n1, n2, s0, s1, s2, float(level), _lib.ptr(ws), ws_bytes)
    _lib.check(L.sdfr_mc_count(*args, counts, st), "marching_cubes")
    nv, nf = int(counts[0]), int(counts[1])
    if nv == 0:
        raise ValueError("Surface level must be within volume data range.")
    verts = torch.empty(nv, 3, dtype=torch.float32, device=volume.device)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=volume.device)
    _lib.check(L.sdfr_mc_emit(*args, _lib.ptr(verts), _lib.ptr(faces), st), "marching_cubes")
    return verts, faces


def extract_mesh_with_marching_cubes(sdf: torch.Tensor) -> Mesh:
    """Zero level set of an aligned SDF volume [1, H, W, D, 1] (sdf_utils.py:188-205):
    the volume read as (x, y, z) = (W, H, D) (the reference's permute(1, 0, 2), here
    a stride swap), vertices scaled to (v / size - 0.5) * 0.24 per axis and y, z
    negated.  A host tensor is moved to the GPU (the reference's caller passes one,
    sdf_mesh.py:153-170)."""
    b, h, w, d, _ = sdf.shape
    vol = sdf[0, ..., 0]
    if not vol.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("extract_mesh_with_marching_cubes: needs the GPU (HIP kernel)")
        vol = vol.to("cuda")
    verts, faces = marching_cubes(vol.permute(1, 0, 2), 0.0)
    for axis, size in enumerate((w, h, d)):
        verts[:, axis] = (verts[:, axis] / float(size) - 0.5) * 0.24
    verts[:, 2] *= -1
    verts[:, 1] *= -1
    return Mesh(verts.cpu().numpy(), faces.cpu().numpy())


def cube_axis(res: int, device=None) -> torch.Tensor:
    """The 1-D table c [res] behind ``cube_points``: c(i) = 2 i / res - 1, formed as
    ``arange * 2 / res - 1`` in fp32 on ``device``."""
    return torch.arange(res, dtype=torch.float32, device=device) * 2 / res - 1


def cube_points(res: int, device=None) -> torch.Tensor:
    """Network coordinates [res, res, res, 3] of the cube ``extract_mesh_with_marching_cubes``
    reads: layout [H (iy), W (ix), D (iz)], and with c(i) = 2 i / res - 1 the point of
    index (iy, ix, iz) is (c(ix), -c(iy), -c(iz)) -- the network coordinate
    (``world_to_network``) of the world position that function gives index (ix, iy, iz):
    (i / res - 0.5) * 0.24 per axis, y and z negated."""
    c = cube_axis(res, device)
    yy, xx, zz = torch.meshgrid(-c, c, -c, indexing="ij")
    return torch.stack([xx, yy, zz], -1)


def world_to_network(v, near: float = 0.88, far: float = 1.12):
    """World position -> what the field network receives under z-normalisation
    (normalized_pts = pts * 2 / (far - near), sdf_model.py:349)."""
    return v * 2 / (far - near)


def sdf_cube(renderer, styles: torch.Tensor, res: int = 128) -> torch.Tensor:
    """The SDF of the field itself on ``cube_points(res)``: [B, res, res, res, 1], which
    goes straight into ``extract_mesh_with_marching_cubes`` (one face at a time) --
    where sdf_mesh.py renders a res^2 x res frustum with return_sdf and resamples it
    trilinearly onto the cube (``align_volume``).  ``styles`` [B, 256]: the renderer's
    latent."""
    B = styles.shape[0]
    pts = cube_points(res, styles.device).reshape(1, res ** 3, 3).expand(B, res ** 3, 3)
    sdf, _ = renderer.query(pts, styles, return_rgb=False)
    return sdf.reshape(B, res, res, res, 1)


class SparseVolume:
    """Narrow-band brick storage of an SDF on a ``res``^3 grid (include/sdfr.h, "Sparse
    marching cubes"): ``slots`` [nb^3] int32 (slot of brick q = (bx nb + by) nb + bz, or
    -1), ``seeds`` and ``surface`` [nb^3] uint8 (the bricks triangulated first, and in the
    end), ``values`` [n_bricks, 8, 8, 8] fp32, ``grow`` [nb^3] uint8 (the last round's leak flags: all zero
    after a completed growth), ``rounds`` (evaluate / classify rounds) and
    ``stored_fraction`` = n_bricks / nb^3."""

    def __init__(self, res, level, slots, seeds, surface, values, grow, rounds):
        self.res, self.level = int(res), float(level)
        self.seeds = seeds
        self.slots, self.surface, self.values, self.grow = slots, surface, values, grow
        self.n_bricks = int(values.shape[0])
        self.rounds = int(rounds)
        self.stored_fraction = self.n_bricks / float((self.res // 8) ** 3)

    def dense(self, fill: float = float("nan")) -> torch.Tensor:
        """The stored values on the full grid [res, res, res] (index (ix, iy, iz)), ``fill``
        wherever no brick is stored.  res^3 floats: for small ``res``, tests and debugging."""
        nb = self.res // 8
        vol = torch.full((nb ** 3, 8, 8, 8), fill, dtype=torch.float32, device=self.values.device)
        stored = self.slots >= 0
        vol[stored] = self.values[self.slots[stored].long()]
        return vol.view(nb, nb, nb, 8, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape((self.res,) * 3)


def _check_brick_res(res: int, what: str) -> int:
    if res < 16 or res % 8 != 0 or res > 2048:
        raise ValueError(f"{what}: res must be a multiple of 8 in [16, 2048], not {res}")
    return res // 8


def sparse_extract(evaluate, axes, res: int, seeds: torch.Tensor, level: float = 0.0,
                   grow: bool = True):
    """Marching cubes on the bricks the surface passes through, never on the full grid:
    ``(verts [V, 3] fp32 in global index coordinates, faces [F, 3] int32, SparseVolume)``,
    all on the GPU (csrc/mesh_sparse.hip).

    ``axes`` = (ax, ay, az), fp32 [res] tables on the GPU: grid point (ix, iy, iz) is
    (ax[ix], ay[iy], az[iz]).  ``evaluate(points [P, 3]) -> [P]`` gives the field there
    (P = 512 per new brick).  ``seeds`` [nb^3] (or [nb, nb, nb], nb = res / 8; bool or
    uint8, GPU): the bricks (bx, by, bz) to triangulate first.  Per round: the seeds' cells
    read K + {0,1}^3, so those bricks get slots (``sdfr_brick_layout``), their points are
    generated (``sdfr_brick_points``) and evaluated -- the new slots only -- and
    ``sdfr_mc_sparse_count`` classifies and flags every brick into which the surface
    leaves through a cell face.  With ``grow`` those bricks join and the round repeats
    until none is flagged: every surface component that touches a seed brick comes out
    completely, equal to the dense mesh's triangles there; a component that lies entirely
    inside bricks never reached is not found.  Without ``grow``: one round, the flags in
    ``SparseVolume.grow``.  ValueError when no edge crosses ``level`` (as
    ``marching_cubes``); RuntimeError for CPU tensors."""
    from . import _lib
    nb = _check_brick_res(res, "sparse_extract")
    if len(axes) != 3 or any(a.shape != (res,) for a in axes):
        raise ValueError(f"sparse_extract: axes must be three [{res}] tables")
    if seeds.numel() != nb ** 3:
        raise ValueError(f"sparse_extract: seeds must have {nb}^3 elements")
    if not seeds.is_cuda or not all(a.is_cuda for a in axes):
        raise RuntimeError("sparse_extract: axes and seeds must be on the GPU (HIP kernels)")
    dev = seeds.device
    L = _lib.lib()
    st = _lib.stream_of(seeds)
    ax, ay, az = (a.to(dev, torch.float32).contiguous() for a in axes)
    seeds = seeds.reshape(-1).ne(0).to(torch.uint8)
    surface = seeds.clone()
    slots = torch.full((nb ** 3,), -1, dtype=torch.int32, device=dev)
    flags = torch.zeros(nb ** 3, dtype=torch.uint8, device=dev)
    lay_bytes = L.sdfr_brick_layout_workspace_bytes(nb)
    lay_ws = torch.empty(lay_bytes, dtype=torch.uint8, device=dev)
    values = torch.empty(0, 8, 8, 8, dtype=torch.float32, device=dev)
    total, counts = _lib._u32(0), (_lib._u32 * 2)()
    n, rounds = 0, 0
    while True:
        _lib.check(L.sdfr_brick_layout(_lib.ptr(surface), nb, _lib.ptr(slots), n,
                                       _lib.ptr(lay_ws), lay_bytes, total, st), "sparse_extract")
        n_new = int(total.value)
        if n_new == 0:
            raise ValueError("Surface level must be within volume data range.")
        if n_new > n:
            pts = torch.empty((n_new - n) * 512, 3, dtype=torch.float32, device=dev)
            _lib.check(L.sdfr_brick_points(_lib.ptr(slots), nb, n, n_new, _lib.ptr(ax),
                                           _lib.ptr(ay), _lib.ptr(az), _lib.ptr(pts), st),
                       "sparse_extract")
            new = evaluate(pts).to(torch.float32).reshape(n_new - n, 8, 8, 8)
            del pts
            values = torch.cat([values, new]) if n else new.contiguous()
            del new
            n = n_new
        rounds += 1
        ws_bytes = L.sdfr_mc_sparse_workspace_bytes(n)
        if ws_bytes == 0:
            raise ValueError(f"sparse_extract: {n} bricks are too many (4 * 512 n + 1 must "
                             "fit 32 bits)")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        args = (_lib.ptr(values), _lib.ptr(slots), _lib.ptr(surface), nb, n, float(level),
                _lib.ptr(ws), ws_bytes)
        _lib.check(L.sdfr_mc_sparse_count(*args, _lib.ptr(flags), counts, st), "sparse_extract")
        if not grow or not bool(flags.any()):
            break
        surface |= flags
        del ws
    volume = SparseVolume(res, level, slots, seeds, surface, values, flags, rounds)
    nv, nf = int(counts[0]), int(counts[1])
    if nv == 0:
        raise ValueError("Surface level must be within volume data range.")
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    _lib.check(L.sdfr_mc_sparse_emit(*args, _lib.ptr(verts), _lib.ptr(faces), st),
               "sparse_extract")
    return verts, faces, volume


Components = namedtuple("Components", ("comp", "n_vertices", "n_faces", "bbox", "area", "count"))
Components.__doc__ = """The connected components of a mesh (``mesh_components``): ``comp`` [V]
int32, the dense id of every vertex's component -- ids 0..count-1 in increasing order of the
component's smallest vertex index; per component ``n_vertices`` and ``n_faces`` [C] int64,
``bbox`` [C, 6] fp32 (min x y z, max x y z over its vertices) and ``area`` [C] float64."""

_SELECTORS = ("keep", "largest", "min_faces", "min_area_frac")


def _cc_check(rc: int, what: str):
    """``_lib.check``, with the device-side findings (a bad face index) as ValueError."""
    from . import _lib
    if rc == _lib.SDFR_EINVAL:
        msg = _lib.lib().sdfr_last_error().decode(errors="replace")
        if "outside [0," in msg:
            raise ValueError(f"{what}: {msg}")
    _lib.check(rc, what)


def _cc_inputs(what, mesh_or_verts, faces):
    """-> (verts [V, 3] fp32 GPU, faces [F, 3] int32 GPU, the Mesh or None)."""
    mesh = mesh_or_verts if isinstance(mesh_or_verts, Mesh) else None
    if mesh is not None:
        if faces is not None:
            raise ValueError(f"{what}: give a Mesh, or vertices and faces")
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what}: needs the GPU (HIP kernels)")
        verts = torch.from_numpy(mesh.vertices).to("cuda")
        faces = torch.from_numpy(mesh.faces).to("cuda")
    else:
        verts = mesh_or_verts
        if not torch.is_tensor(verts) or not torch.is_tensor(faces):
            raise ValueError(f"{what}: give a Mesh, or vertices and faces as tensors")
        if not verts.is_cuda or not faces.is_cuda:
            raise RuntimeError(f"{what}: vertices and faces must be on the GPU (HIP kernels)")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise ValueError(f"{what}: vertices must be [V, 3] with V >= 1, got {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be [F, 3], got {tuple(faces.shape)}")
    V, F = verts.shape[0], faces.shape[0]
    if V >= 2 ** 31 or 3 * F >= 2 ** 31:
        raise ValueError(f"{what}: V and 3 F must be below 2^31")
    if faces.dtype == torch.int64:
        if F:
            lo, hi = (int(x) for x in faces.aminmax())
            if lo < 0 or hi >= V:
                raise ValueError(f"{what}: a face index is outside [0, V) ({lo} .. {hi}, V = {V})")
        faces = faces.to(torch.int32)
    elif faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be int32 or int64, not {faces.dtype}")
    return verts.to(torch.float32).contiguous(), faces.contiguous(), mesh


def _cc_workspace(verts, faces):
    from . import _lib
    n = _lib.lib().sdfr_mesh_cc_workspace_bytes(verts.shape[0], faces.shape[0])
    return torch.empty(n, dtype=torch.uint8, device=verts.device), n


def label_components(faces: torch.Tensor, n_vertices: int):
    """``(label [V] int32, comp [V] int32, count)`` of the faces [F, 3] int32 (GPU) of a mesh
    with ``n_vertices`` vertices (``sdfr_mesh_cc_label``, csrc/mesh_cc.hip): ``label[v]`` is the
    smallest vertex index of v's component, ``comp[v]`` its dense id (components in increasing
    order of their smallest vertex).  Both are pure functions of the mesh.  ValueError for a
    face index outside [0, V): the kernel skips such a face, it is never dereferenced."""
    from . import _lib
    V, F = int(n_vertices), faces.shape[0]
    L = _lib.lib()
    n = L.sdfr_mesh_cc_workspace_bytes(V, F)
    ws = torch.empty(n, dtype=torch.uint8, device=faces.device)
    label = torch.empty(V, dtype=torch.int32, device=faces.device)
    comp = torch.empty(V, dtype=torch.int32, device=faces.device)
    count = _lib._u32(0)
    _cc_check(L.sdfr_mesh_cc_label(_lib.ptr(faces), V, F, _lib.ptr(label), _lib.ptr(comp),
                                   _lib.ptr(ws), n, count, _lib.stream_of(faces)),
              "label_components")
    return label, comp, int(count.value)


def component_stats(verts: torch.Tensor, faces: torch.Tensor, comp: torch.Tensor, count: int):
    """``(n_vertices [C] int32, n_faces [C] int32, bbox [C, 6] fp32, area_q [C] int64, unit)``
    of the components ``comp`` / ``count`` of ``label_components`` (``sdfr_mesh_cc_stats``):
    integer atomics only, so every tensor is reproducible bit for bit.  The area of component
    c is ``area_q[c] * unit`` (unsigned fixed point, below 2^62, in an int64 tensor); ``unit``
    is the power of two include/sdfr.h derives from the bounding box and F, and
    ``|area_q[c] * unit - exact| <= n_faces[c] * unit / 2 + 2^11 * unit``."""
    from . import _lib
    L = _lib.lib()
    dev = verts.device
    V, F, C = verts.shape[0], faces.shape[0], int(count)
    ws, n = _cc_workspace(verts, faces)
    nv = torch.empty(C, dtype=torch.int32, device=dev)
    nf = torch.empty(C, dtype=torch.int32, device=dev)
    bbox = torch.empty(C, 6, dtype=torch.float32, device=dev)
    area_q = torch.empty(C, dtype=torch.int64, device=dev)
    unit = ctypes.c_double(0.0)
    _cc_check(L.sdfr_mesh_cc_stats(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(comp), V, F, C,
                                   _lib.ptr(nv), _lib.ptr(nf), _lib.ptr(bbox), _lib.ptr(area_q),
                                   unit, _lib.ptr(ws), n, _lib.stream_of(verts)),
              "component_stats")
    return nv, nf, bbox, area_q, float(unit.value)


def _components(verts, faces):
    _, comp, count = label_components(faces, verts.shape[0])
    nv, nf, bbox, area_q, unit = component_stats(verts, faces, comp, count)
    return Components(comp, nv.long(), nf.long(), bbox, area_q.double() * unit, count)


def mesh_components(mesh_or_verts, faces=None) -> Components:
    """The connected components of a triangle mesh, on the GPU (csrc/mesh_cc.hip: a lock-free
    union-find over the face edges, then integer-atomic statistics) -- what users of the
    reference get from trimesh's ``mesh.split()``.  A ``Mesh`` (host arrays: moved to the GPU,
    results as NumPy arrays), or ``verts`` [V, 3] fp32 and ``faces`` [F, 3] int32 | int64 on
    the GPU (results stay there).  Two vertices are connected when a face references both; a
    vertex no face references is a component of its own with 0 faces.  Ids run in increasing
    order of the components' smallest vertex index, and every result is reproducible bit for
    bit.  ValueError for a face index outside [0, V) (or an int64 one that does not fit);
    there is no CPU path."""
    verts, faces, mesh = _cc_inputs("mesh_components", mesh_or_verts, faces)
    c = _components(verts, faces)
    if mesh is None:
        return c
    return Components(*(t.cpu().numpy() for t in c[:5]), c.count)


def _keep_mask(c: Components, keep, largest, min_faces, min_area_frac, by):
    dev = c.comp.device
    if keep is not None:
        keep = torch.as_tensor(keep).to(dev)
        if keep.shape != (c.count,):
            raise ValueError(f"keep_components: keep must be [C] = [{c.count}], got "
                             f"{tuple(keep.shape)}")
        return keep.ne(0)
    if largest is not None:
        k = int(largest)
        if k < 1:
            raise ValueError("keep_components: largest must be >= 1")
        size = c.area if by == "area" else c.n_faces
        order = torch.sort(size, descending=True, stable=True).indices   # ties: lower id first
        mask = torch.zeros(c.count, dtype=torch.bool, device=dev)
        mask[order[:k]] = True
        return mask
    if min_faces is not None:
        return c.n_faces >= int(min_faces)
    return c.area >= float(min_area_frac) * c.area.sum()


def keep_components(mesh_or_verts, faces=None, *, keep=None, largest=None, min_faces=None,
                    min_area_frac=None, by="area", drop_unreferenced=True):
    """The mesh without the components that are not wanted, compacted on the GPU
    (``sdfr_mesh_cc_select_count`` / ``_emit``).  Exactly one selector: ``keep`` (bool [C], by
    the ids of ``mesh_components``), ``largest=k`` (the k largest by ``by``: "area" or
    "faces"; ties go to the lower id), ``min_faces`` (components with at least that many
    faces) or ``min_area_frac`` (with at least that fraction of the total area).
    ``drop_unreferenced`` also drops the vertices of kept components that no face references.
    Kept vertices and faces keep their original relative order, so keeping everything on a
    mesh without unreferenced vertices returns arrays equal to the input.

    A ``Mesh`` gives a new ``Mesh`` with ``vertex_colors`` / ``vertex_normals`` carried along;
    GPU tensors give ``(verts [V', 3], faces [F', 3] int32, index_map [V'] int32)``, all on
    the GPU, ``index_map`` new -> old vertex.  ValueError when nothing would be kept."""
    from . import _lib
    given = [n for n, v in zip(_SELECTORS, (keep, largest, min_faces, min_area_frac))
             if v is not None]
    if len(given) != 1:
        raise ValueError("keep_components: give exactly one of keep, largest, min_faces, "
                         f"min_area_frac (got {', '.join(given) or 'none'})")
    if by not in ("area", "faces"):
        raise ValueError(f"keep_components: by must be 'area' or 'faces', not {by!r}")
    if keep is not None:
        # (C is known only after the labelling; a mesh has between 1 and V components)
        n_verts = len(mesh_or_verts.vertices if isinstance(mesh_or_verts, Mesh)
                      else mesh_or_verts)
        shape = tuple(keep.shape) if torch.is_tensor(keep) else np.asarray(keep).shape
        if len(shape) != 1 or not 1 <= shape[0] <= max(n_verts, 1):
            raise ValueError("keep_components: keep must be [C], one entry per component (at "
                             f"most V = {n_verts}), got shape {shape}")
    verts, faces, mesh = _cc_inputs("keep_components", mesh_or_verts, faces)
    c = _components(verts, faces)
    mask = _keep_mask(c, keep, largest, min_faces, min_area_frac, by)
    if not bool(mask.any()):
        raise ValueError("keep_components: no component would be kept")
    mask = mask.to(torch.uint8).contiguous()
    L = _lib.lib()
    st = _lib.stream_of(verts)
    V, F = verts.shape[0], faces.shape[0]
    ws, n = _cc_workspace(verts, faces)
    counts = (_lib._u32 * 2)()
    _cc_check(L.sdfr_mesh_cc_select_count(_lib.ptr(faces), _lib.ptr(c.comp), _lib.ptr(mask), V, F,
                                          c.count, int(bool(drop_unreferenced)), _lib.ptr(ws), n,
                                          counts, st), "keep_components")
    nv, nf = int(counts[0]), int(counts[1])
    if nv == 0:
        raise ValueError("keep_components: no vertex would be kept")
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=verts.device)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=verts.device)
    index_map = torch.empty(nv, dtype=torch.int32, device=verts.device)
    _cc_check(L.sdfr_mesh_cc_select_emit(_lib.ptr(verts), _lib.ptr(faces), V, F, nv, nf,
                                         _lib.ptr(ws), n, _lib.ptr(out_v), _lib.ptr(out_f),
                                         _lib.ptr(index_map), st), "keep_components")
    if mesh is None:
        return out_v, out_f, index_map
    im = index_map.cpu().numpy()
    return Mesh(out_v.cpu().numpy(), out_f.cpu().numpy(),
                None if mesh.vertex_colors is None else mesh.vertex_colors[im],
                None if mesh.vertex_normals is None else mesh.vertex_normals[im])


Simplified = namedtuple("Simplified", ("verts", "faces", "index_map", "cluster", "members"))
Simplified.__doc__ = """A mesh simplified by vertex clustering (``simplify_mesh``), on the GPU:
``verts`` [V', 3] fp32, ``faces`` [F', 3] int32, ``index_map`` [V'] int32 (new vertex -> the
smallest old vertex of its cluster: the map that carries attributes), ``cluster`` [V] int32 (old
vertex -> new vertex, or -1 when its cluster was dropped) and ``members`` [V'] int32 (vertices
merged into each new one)."""

_MAX_SIMPLIFY_DIM = 2 ** 21


def simplify_grid(lo, hi, cell=None, cells=None):
    """The default grid of ``simplify_mesh`` for a bounding box ``lo`` .. ``hi`` (three numbers
    each): ``(origin, cell, dims)``.  The origin is ``lo``; ``cell`` is the given edge length,
    or with ``cells`` the longest edge of the box divided by ``cells``, rounded to fp32;
    ``dims[k] = floor((hi[k] - lo[k]) / cell) + 1`` (in Python floats, from that fp32 cell).
    ValueError unless exactly one of ``cell`` / ``cells`` is given, for a box or cell that is
    not finite, a cell that is not positive, or a grid finer than 2^21 cells along an axis."""
    if (cell is None) == (cells is None):
        raise ValueError("simplify_mesh: give exactly one of cell (the edge length) and cells "
                         "(the number of cells along the longest edge of the bounding box)")
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3 or not np.isfinite(lo + hi).all():
        raise ValueError("simplify_mesh: a vertex coordinate is not finite")
    extent = [h - l for l, h in zip(lo, hi)]
    if cells is not None:
        if not np.isfinite(cells) or cells <= 0:
            raise ValueError(f"simplify_mesh: cells must be a positive number, not {cells!r}")
        cell = max(extent) / float(cells)
    cell = float(np.float32(cell)) if np.isfinite(cell) else float("nan")
    if not np.isfinite(cell) or cell <= 0:
        raise ValueError(f"simplify_mesh: the cell edge must be finite and > 0, not {cell!r}"
                         + (" (the bounding box has no extent)" if cells is not None else ""))
    dims = tuple(int(e / cell) + 1 for e in extent)          # (e >= 0: int() is floor)
    _check_simplify_dims(dims)
    return tuple(lo), cell, dims


def _check_simplify_dims(dims):
    if len(dims) != 3 or any(int(d) != d or not 1 <= d <= _MAX_SIMPLIFY_DIM for d in dims):
        raise ValueError(f"simplify_mesh: dims must be three integers in [1, 2^21], got {dims} "
                         "(a finer grid needs a larger cell)")


def _simplify_check(rc: int, what: str):
    """``_lib.check``, with the device-side findings as ValueError."""
    from . import _lib
    if rc == _lib.SDFR_EINVAL:
        msg = _lib.lib().sdfr_last_error().decode(errors="replace")
        if "outside [0," in msg or "not finite" in msg:
            raise ValueError(f"{what}: {msg}")
    _lib.check(rc, what)


def simplify_mesh(mesh_or_verts, faces=None, *, cell=None, cells=None, origin=None, dims=None,
                  drop_unreferenced=True):
    """The mesh simplified by vertex clustering on a uniform grid, on the GPU
    (csrc/mesh_simplify.hip, ``sdfr_mesh_simplify_count`` / ``_emit``; include/sdfr.h, "Mesh
    simplification") -- where users of the reference decimate with trimesh on the host.  All
    vertices of one grid cell become one vertex at their mean (quantised to 2^-20 of the cell,
    so the result is reproducible bit for bit); a face whose corners no longer differ is
    dropped, and of faces with the same three vertices the first is kept.

    Exactly one of ``cell`` (the cell's edge length) and ``cells`` (the number of cells along
    the longest edge of the bounding box).  ``origin`` (three numbers) and ``dims`` (three
    integers in [1, 2^21]) fix the grid; without them the origin is the bounding box's minimum
    and ``dims[k] = floor(extent[k] / cell) + 1`` (``simplify_grid``).  A vertex outside the
    grid belongs to the nearest boundary cell.  ``drop_unreferenced`` drops the new vertices
    that no kept face references.

    A ``Mesh`` (host arrays) gives a new ``Mesh``; its ``vertex_colors`` / ``vertex_normals``
    are those of each cluster's representative (``[index_map]``) -- call ``color_mesh`` /
    ``normal_mesh`` again for the field's exact values at the new vertices.  ``verts`` [V, 3]
    fp32 and ``faces`` [F, 3] int32 | int64 on the GPU give a ``Simplified`` named tuple, all
    on the GPU.

    Not promised: manifoldness (clustering can pinch thin parts) and feature preservation (the
    mean pulls a convex surface inwards, by less than one cell).  Guaranteed for vertices
    inside the grid: a vertex and the new vertex of its cluster lie in one cell.

    ValueError for bad selectors, a face index outside [0, V), a non-finite coordinate, or
    when no face survives with ``drop_unreferenced`` (the cell is too coarse for the mesh).
    There is no CPU path."""
    from . import _lib
    what = "simplify_mesh"
    if (cell is None) == (cells is None):
        raise ValueError("simplify_mesh: give exactly one of cell (the edge length) and cells "
                         "(the number of cells along the longest edge of the bounding box)")
    if cell is not None and not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"simplify_mesh: the cell edge must be finite and > 0, not {cell!r}")
    if cells is not None and not (np.isfinite(cells) and cells > 0):
        raise ValueError(f"simplify_mesh: cells must be a positive number, not {cells!r}")
    if origin is not None:
        origin = tuple(float(x) for x in origin)
        if len(origin) != 3 or not np.isfinite(origin).all():
            raise ValueError(f"simplify_mesh: origin must be three finite numbers, got {origin}")
    if dims is not None:
        dims = tuple(dims)
        _check_simplify_dims(dims)
    verts, faces, mesh = _cc_inputs(what, mesh_or_verts, faces)
    if origin is None or dims is None or cells is not None:
        lo, hi = (t.cpu().tolist() for t in verts.aminmax(dim=0))
        _, cell, box_dims = simplify_grid(lo, hi, cell, cells)
        if origin is None:
            origin = tuple(lo)
        elif dims is None:                           # the box as seen from the given origin
            box_dims = simplify_grid(origin, [max(h, o) for h, o in zip(hi, origin)],
                                     cell=cell)[2]
        dims = box_dims if dims is None else dims
    L = _lib.lib()
    st = _lib.stream_of(verts)
    dev = verts.device
    V, F = verts.shape[0], faces.shape[0]
    n = L.sdfr_mesh_simplify_workspace_bytes(V, F)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = (_lib._u32 * 3)()
    _simplify_check(L.sdfr_mesh_simplify_count(
        _lib.ptr(verts), _lib.ptr(faces), V, F, origin[0], origin[1], origin[2], float(cell),
        int(dims[0]), int(dims[1]), int(dims[2]), int(bool(drop_unreferenced)), _lib.ptr(ws), n,
        counts, st), what)
    nv, nf = int(counts[1]), int(counts[2])
    if nv == 0:
        raise ValueError("simplify_mesh: no face survives: the cell is too coarse for this mesh "
                         f"({int(counts[0])} clusters; pass drop_unreferenced=False to get them)")
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    index_map = torch.empty(nv, dtype=torch.int32, device=dev)
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    members = torch.empty(nv, dtype=torch.int32, device=dev)
    _simplify_check(L.sdfr_mesh_simplify_emit(
        _lib.ptr(verts), _lib.ptr(faces), V, F, nv, nf, _lib.ptr(ws), n, _lib.ptr(out_v),
        _lib.ptr(out_f), _lib.ptr(index_map), _lib.ptr(cluster), _lib.ptr(members), st), what)
    if mesh is None:
        return Simplified(out_v, out_f, index_map, cluster, members)
    im = index_map.cpu().numpy()
    return Mesh(out_v.cpu().numpy(), out_f.cpu().numpy(),
                None if mesh.vertex_colors is None else mesh.vertex_colors[im],
                None if mesh.vertex_normals is None else mesh.vertex_normals[im])


def _check_simplify_factor(simplify, what):
    if simplify is None:
        return None
    if isinstance(simplify, bool) or int(simplify) != simplify or simplify < 2:
        raise ValueError(f"{what}: simplify must be None or an integer >= 2 (lattice cells per "
                         f"cluster cell), not {simplify!r}")
    return int(simplify)


Smoothed = namedtuple("Smoothed", ("verts", "valence", "boundary"))
Smoothed.__doc__ = """A mesh smoothed on the GPU (``smooth_mesh``): ``verts`` [V, 3] fp32 (the
faces are the input's), ``valence`` [V] int32 (face corners per vertex) and ``boundary`` [V]
bool (the vertex is an end of an edge that exactly one face has)."""

_SMOOTH_UNIT_LOG2 = (-126, 96)


def smooth_lattice(lo, hi):
    """The default lattice of ``smooth_mesh`` for a bounding box ``lo`` .. ``hi`` (three numbers
    each, fp32 values): ``(origin, unit_log2)``.  The origin is ``lo``; with E the longest
    edge of the box (in float64; 0 is taken as 1) written as m 2^x, m in [0.5, 1),
    ``unit_log2 = x - 30``: the box spans at most 2^30 units of 2^unit_log2.  ValueError for a
    box that is not finite, or whose unit would leave [-126, 96]."""
    import math
    lo = [float(np.float32(x)) for x in lo]
    hi = [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3 or not np.isfinite(lo + hi).all():
        raise ValueError("smooth_mesh: a vertex coordinate is not finite")
    extent = max(h - l for l, h in zip(lo, hi))
    if not extent > 0:
        extent = 1.0
    unit_log2 = math.frexp(extent)[1] - 30
    _check_smooth_unit(unit_log2)
    return tuple(lo), unit_log2


def _check_smooth_unit(unit_log2):
    if isinstance(unit_log2, bool) or int(unit_log2) != unit_log2 or \
            not _SMOOTH_UNIT_LOG2[0] <= unit_log2 <= _SMOOTH_UNIT_LOG2[1]:
        raise ValueError(f"smooth_mesh: unit_log2 must be an integer in [-126, 96], not "
                         f"{unit_log2!r}")


def _smooth_check(rc: int, what: str):
    """``_lib.check``, with the device-side findings as ValueError."""
    from . import _lib
    if rc == _lib.SDFR_EINVAL:
        msg = _lib.lib().sdfr_last_error().decode(errors="replace")
        if "outside [0," in msg or "not finite" in msg or "outside the lattice" in msg:
            raise ValueError(f"{what}: {msg}")
    _lib.check(rc, what)


def _smooth_schedule(iterations, lam, mu):
    """The pass weights of ``smooth_mesh``: ``iterations`` times (lam,) or (lam, mu)."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) \
            or iterations < 0:
        raise ValueError(f"smooth_mesh: iterations must be an integer >= 0, not {iterations!r}")
    if not (np.isfinite(lam) and 0 < lam <= 1):
        raise ValueError(f"smooth_mesh: lam must be in (0, 1], not {lam!r}")
    if mu is not None and not (np.isfinite(mu) and -1 <= mu <= 0):
        raise ValueError(f"smooth_mesh: mu must be None or in [-1, 0], not {mu!r}")
    one = [float(lam)] if mu is None or mu == 0 else [float(lam), float(mu)]
    weights = one * int(iterations)
    if len(weights) > 1024:
        raise ValueError(f"smooth_mesh: {len(weights)} passes; at most 1024 in one call")
    return weights


def _smooth_prepare(what, verts, faces, origin, unit_log2, pin_boundary):
    """``sdfr_mesh_smooth_prepare`` -> (workspace, its size, valence, boundary)."""
    from . import _lib
    if (origin is None) != (unit_log2 is None):
        raise ValueError(f"{what}: give both origin and unit_log2 (the lattice), or neither")
    if origin is None:
        lo, hi = (t.cpu().tolist() for t in verts.aminmax(dim=0))
        origin, unit_log2 = smooth_lattice(lo, hi)
    else:
        origin = tuple(float(x) for x in origin)
        if len(origin) != 3 or not np.isfinite(origin).all():
            raise ValueError(f"{what}: origin must be three finite numbers, got {origin}")
        _check_smooth_unit(unit_log2)
    L = _lib.lib()
    dev = verts.device
    V, F = verts.shape[0], faces.shape[0]
    n = L.sdfr_mesh_smooth_workspace_bytes(V, F)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    valence = torch.empty(V, dtype=torch.int32, device=dev)
    boundary = torch.empty(V, dtype=torch.bool, device=dev)
    _smooth_check(L.sdfr_mesh_smooth_prepare(
        _lib.ptr(verts), _lib.ptr(faces), V, F, origin[0], origin[1], origin[2], int(unit_log2),
        int(bool(pin_boundary)), _lib.ptr(ws), n, _lib.ptr(valence), _lib.ptr(boundary),
        _lib.stream_of(verts)), what)
    return ws, n, valence, boundary


def mesh_boundary(mesh_or_verts, faces=None):
    """``(valence, boundary)`` of a mesh, on the GPU (``sdfr_mesh_smooth_prepare`` alone):
    ``valence`` [V] int32, the number of face corners at each vertex, and ``boundary`` [V]
    bool, whether the vertex is an end of an edge that exactly one face has.
    ``boundary.any()`` answers "is this mesh open?" -- for the field's mesh, whether the level
    set left the cube.  A ``Mesh`` gives NumPy arrays, device tensors give device tensors.
    ValueError for a face index outside [0, V) or a non-finite coordinate."""
    what = "mesh_boundary"
    verts, faces, mesh = _cc_inputs(what, mesh_or_verts, faces)
    _, _, valence, boundary = _smooth_prepare(what, verts, faces, None, None, True)
    if mesh is None:
        return valence, boundary
    return valence.cpu().numpy(), boundary.cpu().numpy()


def smooth_mesh(mesh_or_verts, faces=None, *, iterations=10, lam=0.5, mu=-0.53,
                pin_boundary=True, origin=None, unit_log2=None):
    """The mesh smoothed by Laplacian or Taubin lambda | mu passes of the uniform umbrella
    operator, on the GPU (csrc/mesh_smooth.hip, ``sdfr_mesh_smooth_prepare`` / ``_run``;
    include/sdfr.h, "Mesh smoothing") -- where users of the reference call trimesh's
    ``filter_taubin`` / ``filter_laplacian`` on the host.  The vertices are quantised to an
    integer lattice and the passes run on integers, so the result is reproducible bit for
    bit, whatever the order of the faces.

    ``iterations`` times a pass of weight ``lam`` followed by one of weight ``mu`` (Taubin:
    the second pass undoes the shrinkage of the first); ``mu=None`` or ``mu=0`` gives
    Laplacian passes of weight ``lam`` alone.  ``pin_boundary`` keeps the vertices on an open
    mesh's border where they are.  ``origin`` (three numbers) and ``unit_log2`` (an integer in
    [-126, 96]) fix the lattice of spacing 2^unit_log2, on which every vertex must lie within
    [0, 2^30] units of the origin per axis; without them it is ``smooth_lattice`` of the
    bounding box.  ``iterations=0`` returns the input's bits, and a vertex that no face
    references or that is pinned always keeps them.

    A ``Mesh`` (host arrays) gives a new ``Mesh`` with the same faces; its ``vertex_colors`` /
    ``vertex_normals`` are carried over unchanged (the indexing is the same) -- call
    ``color_mesh`` / ``normal_mesh`` again for the field's values at the moved vertices.
    ``verts`` [V, 3] fp32 and ``faces`` [F, 3] int32 | int64 on the GPU give a ``Smoothed``
    named tuple, all on the GPU.

    ValueError for bad selectors (``iterations`` negative or not an integer, ``lam`` not in
    (0, 1], ``mu`` not in [-1, 0]), half a lattice, a face index outside [0, V), a
    non-finite coordinate, or a vertex outside the lattice.  There is no CPU path."""
    from . import _lib
    what = "smooth_mesh"
    weights = _smooth_schedule(iterations, lam, mu)
    verts, faces, mesh = _cc_inputs(what, mesh_or_verts, faces)
    ws, n, valence, boundary = _smooth_prepare(what, verts, faces, origin, unit_log2,
                                               pin_boundary)
    out = torch.empty_like(verts)
    w = (_lib._f32 * max(len(weights), 1))(*weights)
    _smooth_check(_lib.lib().sdfr_mesh_smooth_run(
        _lib.ptr(verts), verts.shape[0], w, len(weights), _lib.ptr(ws), n, _lib.ptr(out),
        _lib.stream_of(verts)), what)
    if mesh is None:
        return Smoothed(out, valence, boundary)
    return Mesh(out.cpu().numpy(), mesh.faces, mesh.vertex_colors, mesh.vertex_normals)


def _check_smooth(smooth, what):
    """``smooth`` of ``sparse_mesh``: None, or the keyword arguments of ``smooth_mesh``."""
    if smooth is None:
        return None
    if isinstance(smooth, dict):
        kw = dict(smooth)
        if "origin" in kw or "unit_log2" in kw:
            raise ValueError(f"{what}: smooth takes no lattice: it is that of res")
    elif isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)):
        raise ValueError(f"{what}: smooth must be None, an integer (Taubin iterations) or a "
                         f"dict of smooth_mesh keyword arguments, not {smooth!r}")
    else:
        kw = {"iterations": int(smooth)}
    _smooth_schedule(kw.get("iterations", 10), kw.get("lam", 0.5), kw.get("mu", -0.53))
    return kw


def sparse_mesh(evaluate, axes, res: int, seeds: torch.Tensor, level: float = 0.0,
                grow: bool = True, components=None, simplify=None, smooth=None):
    """``sparse_extract`` and ``extract_mesh_sparse``'s finish: ``(Mesh, SparseVolume)`` with
    the vertices scaled to (v / res - 0.5) * 0.24 per axis and y, z negated, on the host.
    ``components``: ``None``, or a dict of ``keep_components`` keyword arguments that filters
    the mesh on the GPU before the scaling and before the copy to the host (so only what is
    kept is copied).  ``simplify``: ``None``, or an integer k >= 2: after that filter (a floater
    is never merged into the face) and before the scaling and the copy, ``simplify_mesh`` in
    index coordinates on the grid of origin 0, cell k and ceil(res / k) cells per axis -- a
    function of ``res`` and k alone, not of the mesh.  ``smooth``: ``None``, an integer (that
    many Taubin iterations with ``smooth_mesh``'s defaults) or a dict of ``smooth_mesh``
    keyword arguments: after the two steps above and before the scaling and the copy,
    ``smooth_mesh`` in index coordinates on the lattice ``smooth_lattice((0, 0, 0), (res, res,
    res))`` -- a function of ``res`` alone, so no bounding box is computed."""
    simplify = _check_simplify_factor(simplify, "sparse_mesh")
    smooth = _check_smooth(smooth, "sparse_mesh")
    verts, faces, volume = sparse_extract(evaluate, axes, res, seeds, level, grow)
    if components is not None:
        verts, faces, _ = keep_components(verts, faces, **components)
    if simplify is not None:
        verts, faces = simplify_mesh(verts, faces, cell=float(simplify), origin=(0.0, 0.0, 0.0),
                                     dims=(-(-res // simplify),) * 3)[:2]
    if smooth is not None:
        origin, unit_log2 = smooth_lattice((0.0,) * 3, (float(res),) * 3)
        verts = smooth_mesh(verts, faces, origin=origin, unit_log2=unit_log2, **smooth).verts
    for axis in range(3):
        verts[:, axis] = (verts[:, axis] / float(res) - 0.5) * 0.24
    verts[:, 2] *= -1
    verts[:, 1] *= -1
    return Mesh(verts.cpu().numpy(), faces.cpu().numpy()), volume


def extract_mesh_sparse(renderer, styles: torch.Tensor, res: int = 512, level: float = 0.0,
                        lipschitz=None, grow: bool = True, return_volume: bool = False,
                        components=None, simplify=None, smooth=None):
    """The ``level`` set of the field itself at ``res``^3 without the dense cube: the
    ``Mesh`` that ``extract_mesh_with_marching_cubes(sdf_cube(renderer, styles, res))``
    gives (same vertex scaling and y / z flips, the same triangles with bit-equal
    vertices; their order differs) wherever nothing was skipped -- with the field evaluated
    only on the 8^3-point bricks near the surface (``sparse_extract``), so 1024^3 fits
    where the dense path stops near 640^3.  One face (``styles`` [1, 256]); ``color_mesh``
    and ``normal_mesh`` work on the result.

    Seeds: brick K is one when ``|sdf(centre) - level| <= L * 4 sqrt(3) h`` at its centre,
    the lattice point 8 K + 4 per axis; h = 2 / res is the grid spacing in network
    coordinates and 4 sqrt(3) h the distance from the centre to the farthest corner of the
    brick's cells.  ``lipschitz`` is L; ``None`` takes the maximum of ``|grad sdf|`` over
    the nb^3 centres (``query_gradient``).  That is a sampled estimate, not a bound: the
    field can be steeper between the centres, and then a brick the surface crosses may not
    be a seed.  With ``grow`` every surface component that touches a seed brick is still
    extracted completely, whatever L is; what can be missed is a component that lies
    entirely inside skipped bricks (a small detached blob far from where the SDF is
    small at the centres).  ``return_volume``: also the ``SparseVolume``.

    ``components``: ``None`` (everything found), or a dict of ``keep_components`` keyword
    arguments, e.g. ``{"largest": 1}``: the mesh is split into its connected components and
    filtered on the GPU before the vertex scaling and before the copy to the host, so the
    unwanted components are never copied.  The components' bounding boxes and areas then
    refer to index coordinates (0 .. res - 1 per axis), not to world coordinates.

    ``simplify``: ``None`` (the mesh as extracted), or an integer k >= 2: the mesh is thinned by
    vertex clustering (``simplify_mesh``) with k lattice cells per cluster cell, on the GPU,
    after the ``components`` filter and before the vertex scaling and the copy to the host --
    about 1 / k^2 of the vertices and faces are copied.  The grid depends on ``res`` and k
    only.  Not promised: manifoldness and sharp features (see ``simplify_mesh``).

    ``smooth``: ``None`` (no smoothing), an integer n (n Taubin iterations with
    ``smooth_mesh``'s defaults) or a dict of ``smooth_mesh`` keyword arguments: the mesh is
    smoothed on the GPU after ``components`` and ``simplify`` and before the vertex scaling
    and the copy -- it takes off the facets that clustering prints onto the surface and the
    hash grid's high-frequency bumps.  The lattice depends on ``res`` only."""
    if styles.shape[0] != 1:
        raise ValueError("extract_mesh_sparse: one mesh, one face (styles [1, 256])")
    simplify = _check_simplify_factor(simplify, "extract_mesh_sparse")
    smooth = _check_smooth(smooth, "extract_mesh_sparse")
    nb = _check_brick_res(res, "extract_mesh_sparse")
    if not styles.is_cuda:
        raise RuntimeError("extract_mesh_sparse: needs the GPU (HIP kernels)")
    dev = styles.device
    c = cube_axis(res, dev)
    axes = (c, -c, -c)

    def evaluate(pts):
        return renderer.query(pts.unsqueeze(0), styles, return_rgb=False)[0].reshape(-1)

    with torch.no_grad():
        mid = torch.arange(nb, device=dev) * 8 + 4
        centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"),
                              -1).reshape(1, nb ** 3, 3)
        sdf_c = renderer.query(centres, styles, return_rgb=False)[0]
        if lipschitz is None:
            lipschitz = float(renderer.query_gradient(centres, styles)[1].float()
                              .norm(dim=-1).max())
        band = float(lipschitz) * 4.0 * (3.0 ** 0.5) * (2.0 / res)
        seeds = (sdf_c.reshape(-1).float() - level).abs() <= band
        mesh, volume = sparse_mesh(evaluate, axes, res, seeds, level, grow, components,
                                   simplify, smooth)
    return (mesh, volume) if return_volume else mesh


def color_mesh(mesh: Mesh, renderer, styles: torch.Tensor, viewdir=(0.0, 0.0, -1.0),
               near: float = 0.88, far: float = 1.12) -> np.ndarray:
    """The field's colour at every vertex of ``mesh`` (world coordinates, as
    ``extract_mesh_with_marching_cubes`` returns them) for the face ``styles`` [1, 256],
    seen from ``viewdir``: one unit direction, or [V, 3] one per vertex (as the network
    sees it; not normalised here).  Sets and returns ``mesh.vertex_colors`` [V, 3] in
    [0, 1]."""
    if styles.shape[0] != 1:
        raise ValueError("color_mesh: one mesh, one face (styles [1, 256])")
    dev = styles.device
    pts = world_to_network(torch.as_tensor(mesh.vertices, dtype=torch.float32, device=dev),
                           near, far).unsqueeze(0)
    vd = torch.as_tensor(np.asarray(viewdir, np.float32), device=dev)
    vd = vd.reshape(1, 3) if vd.dim() == 1 else vd.reshape(1, -1, 3)
    with torch.no_grad():
        _, rgb = renderer.query(pts, styles, viewdirs=vd)
    mesh.vertex_colors = rgb[0].float().cpu().numpy()
    return mesh.vertex_colors


def normal_mesh(mesh: Mesh, renderer, styles: torch.Tensor, near: float = 0.88,
                far: float = 1.12) -> np.ndarray:
    """The field's unit normal at every vertex of ``mesh`` (world coordinates) for the
    face ``styles`` [1, 256]: the normalised SDF gradient at ``world_to_network(vertices)``
    -- the positive uniform scale of ``world_to_network`` does not change directions.  The
    SDF grows outward, so the normals point out of the surface.  A vertex where the
    gradient vanishes (outside the hash grid's box) keeps a zero normal.  Sets and returns
    ``mesh.vertex_normals`` [V, 3]."""
    if styles.shape[0] != 1:
        raise ValueError("normal_mesh: one mesh, one face (styles [1, 256])")
    dev = styles.device
    pts = world_to_network(torch.as_tensor(mesh.vertices, dtype=torch.float32, device=dev),
                           near, far).unsqueeze(0)
    with torch.no_grad():
        _, n = renderer.query_gradient(pts, styles, normalize=True)
    mesh.vertex_normals = n[0].float().cpu().numpy()
    return mesh.vertex_normals


def eikonal_residual(renderer, styles: torch.Tensor, points: torch.Tensor, near: float = 0.88,
                     far: float = 1.12) -> torch.Tensor:
    """``|grad_world sdf| - 1`` at ``points`` [B, M, 3] (network coordinates): [B, M], zero
    for a true distance field.  ``query_gradient`` differentiates with respect to the
    network coordinate p = x_world * 2 / (far - near), so
    grad_world = grad_network * 2 / (far - near)."""
    with torch.no_grad():
        _, g = renderer.query_gradient(points, styles)
    return (g * (2 / (far - near))).norm(dim=-1) - 1


def shade_surface(surface, light_dir=(-0.5, 1.0, 5.0), ambient: float = 0.3,
                  albedo=None) -> torch.Tensor:
    """A lit view [B, 3, H, W] of a ``Surface`` (``render_surface`` with ``hit`` and
    ``normal``): ``hit * albedo * (ambient + (1 - ambient) * max(0, n . l))`` with ``l`` the
    unit vector along ``light_dir`` (world coordinates; the default is the location of the
    reference's PointLights, sdf_utils.py:209-331, used as a direction).  ``albedo``
    [B, 3, H, W] or [B, 1, H, W]; ``None`` takes ``surface.rgb``, or white without one.
    Plain torch: one pass over a few maps."""
    if surface.hit is None or surface.normal is None:
        raise ValueError("shade_surface: the surface needs its hit and normal maps")
    n = surface.normal
    l = torch.as_tensor(light_dir, dtype=n.dtype, device=n.device)
    l = (l / l.norm()).view(1, 3, 1, 1)
    if albedo is None:
        albedo = surface.rgb if surface.rgb is not None else torch.ones_like(n)
    lambert = (n * l).sum(1, keepdim=True).clamp_min(0)
    return surface.hit * albedo.expand_as(n) * (ambient + (1 - ambient) * lambert)


def xyz2mesh(xyz: torch.Tensor):
    """Mesh from an expected-surface xyz map [1, 3, H, W] (sdf_utils.py:209):
    Delaunay triangulation of the pixel grid, normals inverted.  Returns
    (vertices [H*W, 3], faces) or a trimesh.Trimesh when trimesh is present."""
    from scipy.spatial import Delaunay
    _, _, h, w = xyz.shape
    x, y = np.meshgrid(np.arange(h), np.arange(w))
    tri = Delaunay(np.concatenate((x.reshape(h * w, 1), y.reshape(h * w, 1)), 1))
    faces = tri.simplices
    faces[:, [0, 1]] = faces[:, [1, 0]]
    verts = xyz.squeeze(0).permute(1, 2, 0).reshape(h * w, 3).cpu().numpy()
    try:
        import trimesh
    except ImportError:
        return verts, faces
    return trimesh.Trimesh(verts, faces)

"""CPU: the mesh rasteriser's definition against an independent float64 ray cast, and the
host-side pieces around it (load_obj, subdivide_mesh, the range check, the C ABI)."""
import io

import numpy as np
import pytest
import torch

from tests import raster_ref as R

# (azimuth, elevation, resolution): look-at cameras at distance 1, focal (res/2)/tan(6 deg)
VIEWS = R.VIEWS
COVERED = (725, 728, 1624)

DEPTH_BOUND, RAY_BOUND = R.DEPTH_BOUND, R.RAY_BOUND


@pytest.fixture(scope="module")
def sphere():
    return R.icosphere(2, 0.1)


@pytest.fixture(scope="module")
def views(sphere):
    """Per view: camera, focal, res, the fp32 reference and the float64 ray cast (computed
    once, read by the tests below)."""
    v, f = sphere
    out = []
    for az, el, res in VIEWS:
        cam, foc = R.look_at(az, el), R.fov_focal(res)
        fi, dep, bar = R.raster_ref(v, f, cam[None], [foc], res, res)
        out.append(dict(cam=cam, focal=foc, res=res, face_idx=fi[0], depth=dep[0], bary=bar[0],
                        ray=R.raycast_ref(v, f, cam, foc, res, res)))
    return out


def test_icosphere_counts(sphere):
    v, f = sphere
    assert v.shape == (162, 3) and f.shape == (320, 3)
    # closed, outward winding: every face normal points away from the centre
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * v[f].mean(1)).sum(-1) > 0).all()


def test_definition_matches_float64_raycast(views):
    for view, n_cov in zip(views, COVERED):
        fi, dep = view["face_idx"], view["depth"]
        rf, rt, rb = view["ray"]
        cov = fi >= 0
        assert np.array_equal(cov, rf >= 0)
        assert int(cov.sum()) == n_cov
        differ = cov & (fi != rf)
        # an id may differ only where the ray passes within 1e-2 (barycentric) of an edge
        assert (np.abs(rb[differ]).min(-1) < 1e-2).all()
        assert int(differ.sum()) <= 0.01 * n_cov
        agree = cov & (fi == rf)
        err = np.abs(dep.astype(np.float64) - rt)[agree].max()
        print(f"res {view['res']}: covered {n_cov}, ids differ {int(differ.sum())}, "
              f"max depth error {err:.3e}")
        assert err <= DEPTH_BOUND
        assert (dep[~cov] == 0).all() and (view["bary"][~cov] == 0).all()


def test_perspective_correct_positions_lie_on_the_ray(sphere, views):
    v, f = sphere
    for view in views:
        fi, dep, bar, res = view["face_idx"], view["depth"], view["bary"], view["res"]
        cov = fi >= 0
        o, d = R.rays_ref(view["cam"], float(np.float32(view["focal"])), res, res)
        on_ray = o + d * dep.astype(np.float64)[..., None]
        xyz = np.moveaxis(R.interp_ref(v, f, fi[None], bar[None])[0], 0, -1)
        err = np.abs(xyz.astype(np.float64) - on_ray).max(-1)[cov].max()
        print(f"res {res}: max |xyz - (o + d depth)| {err:.3e}")
        assert err <= RAY_BOUND
        # screen-space weights (bary_i z_i / depth, renormalised) miss the ray: the check
        # above separates the two
        z = _vertex_depth(v, view["cam"])[f[np.where(cov, fi, 0)]]
        lin = bar.astype(np.float64) * z / np.where(cov, dep, 1).astype(np.float64)[..., None]
        lin /= np.where(cov, lin.sum(-1), 1.0)[..., None]
        flat = (lin[..., None] * v.astype(np.float64)[f[np.where(cov, fi, 0)]]).sum(-2)
        assert np.abs(flat - on_ray).max(-1)[cov].max() > 10 * RAY_BOUND


def _vertex_depth(v, cam):
    cam = cam.astype(np.float64)
    return -((v.astype(np.float64) - cam[:, 3]) @ cam[:, :3])[:, 2]


@pytest.mark.parametrize("colors", (False, True))
@pytest.mark.parametrize("normals", (False, True))
def test_load_obj_round_trip(sdfr, sphere, tmp_path, colors, normals):
    v, f = sphere
    rng = np.random.default_rng(3)
    c = rng.random(v.shape, np.float32) if colors else None
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if normals else None
    mesh = sdfr.Mesh(v, f, vertex_colors=c, vertex_normals=n)
    text = mesh.export()
    path = tmp_path / "m.obj"
    mesh.export(str(path))
    for back in (sdfr.load_obj(io.StringIO(text)), sdfr.load_obj(str(path))):
        assert back.vertices.dtype == np.float32 and back.faces.dtype == np.int64
        assert np.array_equal(back.faces, f)
        # %.8f, then the nearest float32 to the printed number
        assert np.abs(back.vertices - v).max() <= 0.5e-8 + np.spacing(np.abs(v).max()) / 2
        assert (back.vertex_colors is None) == (not colors)
        assert (back.vertex_normals is None) == (not normals)
        if colors:
            assert np.abs(back.vertex_colors - c).max() <= 0.5e-6 + 1e-7   # %.6f
        if normals:
            assert np.abs(back.vertex_normals - n).max() <= 0.5e-6 + 1e-7
        # what was read writes the same text again
        assert sdfr.load_obj(io.StringIO(back.export())).export() == back.export()


def _edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return np.unique(e, axis=0)


@pytest.mark.parametrize("shape", ("tetrahedron", "icosphere"))
def test_subdivide_mesh(sdfr, sphere, shape):
    if shape == "tetrahedron":
        v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
        f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
    else:
        v, f = sphere
    rng = np.random.default_rng(5)
    c = rng.random(v.shape, np.float32)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    mesh = sdfr.Mesh(v, f, vertex_colors=c, vertex_normals=n)
    sub = sdfr.subdivide_mesh(mesh)
    V, F = len(v), len(f)
    e = _edges(f)                                   # ascending (min, max)
    E = len(e)
    assert V - E + F == 2
    assert sub.vertices.shape == (V + E, 3) and sub.faces.shape == (4 * F, 3)
    assert len(sub.vertices) - len(_edges(sub.faces)) + len(sub.faces) == 2
    assert np.array_equal(sub.vertices[:V], v)
    # new vertex V + k is the midpoint of the k-th edge in ascending (min, max) order
    assert np.array_equal(sub.vertices[V:], (v[e[:, 0]] + v[e[:, 1]]) * np.float32(0.5))
    assert np.array_equal(sub.vertex_colors[V:], (c[e[:, 0]] + c[e[:, 1]]) * np.float32(0.5))
    assert np.array_equal(sub.vertex_normals[:V], n)
    assert np.abs(np.linalg.norm(sub.vertex_normals, axis=1) - 1).max() < 1e-6
    mean_n = n[e[:, 0]] + n[e[:, 1]]
    assert np.abs(sub.vertex_normals[V:]
                  - mean_n / np.linalg.norm(mean_n, axis=1, keepdims=True)).max() < 1e-6
    # children of face (a, b, c): [a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]
    index = {tuple(x): V + k for k, x in enumerate(e.tolist())}

    def mid(p, q):
        return index[(min(p, q), max(p, q))]

    want = []
    for a, b, cc in f.tolist():
        ab, bc, ca = mid(a, b), mid(b, cc), mid(cc, a)
        want += [[a, ab, ca], [b, bc, ab], [cc, ca, bc], [ab, bc, ca]]
    assert np.array_equal(sub.faces, np.asarray(want))
    again = sdfr.subdivide_mesh(mesh)
    assert np.array_equal(again.vertices, sub.vertices) and np.array_equal(again.faces, sub.faces)
    twice = sdfr.subdivide_mesh(mesh, 2)
    once_more = sdfr.subdivide_mesh(sub)
    assert np.array_equal(twice.vertices, once_more.vertices)
    assert np.array_equal(twice.faces, once_more.faces)
    assert sdfr.subdivide_mesh(mesh, 0) is mesh


def test_face_index_out_of_range_is_a_host_error(sdfr, sphere):
    v, f = sphere
    bad = f.copy()
    bad[7, 1] = len(v)
    cam = torch.from_numpy(R.look_at(0.0, 0.0))[None]
    with pytest.raises(ValueError, match="face indices"):
        sdfr.rasterize_mesh(sdfr.Mesh(v, bad), cam, 100.0, 16)
    bad[7, 1] = -1
    with pytest.raises(ValueError, match="face indices"):
        sdfr.rasterize_mesh(sdfr.Mesh(v, bad), cam, 100.0, 16)
    # a good mesh gets past the check, to the device requirement
    with pytest.raises(RuntimeError, match="needs the GPU"):
        sdfr.rasterize_mesh(sdfr.Mesh(v, f), cam, 100.0, 16)


def test_raster_c_abi(sdfr):
    lib = sdfr._lib.lib()
    for name in ("sdfr_mesh_raster_workspace_bytes", "sdfr_mesh_raster", "sdfr_mesh_interpolate"):
        assert name in sdfr._lib.EXPORTS and hasattr(lib, name), name
    assert lib.sdfr_abi_version() == 15                      # additive: no version step
    size = lib.sdfr_mesh_raster_workspace_bytes
    # projected vertices 16 B, keys 8 B, counter, list 8 B; each region rounded up to 256
    assert size(2, 32, 48, 162, 320) == 5376 + 2 * 32 * 48 * 8 + 256 + 2 * 320 * 8
    assert size(0, 32, 32, 4, 4) == 0 and size(1, 32, 32, 0, 4) == 0
    assert size(1, 16385, 32, 4, 4) == 0 and size(1 << 20, 64, 64, 4, 4) == 0
    EINVAL = sdfr._lib.SDFR_EINVAL
    assert lib.sdfr_mesh_raster(None, None) == EINVAL
    assert b"null arguments" in lib.sdfr_last_error()
    a = sdfr._lib.RasterArgs(B=1, H=8, W=8, V=3, F=1)
    import ctypes
    assert lib.sdfr_mesh_raster(ctypes.byref(a), None) == EINVAL
    assert b"null vertices" in lib.sdfr_last_error()
    a.B = 0
    assert lib.sdfr_mesh_raster(ctypes.byref(a), None) == EINVAL
    assert b"sizes" in lib.sdfr_last_error()
    # (the checks precede every launch and dereference nothing: any non-null value will do)
    fake = ctypes.c_void_p(256)
    a = sdfr._lib.RasterArgs(B=1, H=8, W=8, V=3, F=1, vertices=fake, faces=fake, cam=fake,
                             focal=fake, cx=4, cy=4, znear=0.01)
    assert lib.sdfr_mesh_raster(ctypes.byref(a), None) == EINVAL
    assert b"every output is null" in lib.sdfr_last_error()
    a.face_idx = fake
    a.workspace, a.workspace_bytes = fake, size(1, 8, 8, 3, 1) - 1
    assert lib.sdfr_mesh_raster(ctypes.byref(a), None) == EINVAL
    assert b"workspace too small" in lib.sdfr_last_error()
    a.workspace_bytes, a.znear = size(1, 8, 8, 3, 1), -1.0
    assert lib.sdfr_mesh_raster(ctypes.byref(a), None) == EINVAL
    assert b"znear" in lib.sdfr_last_error()
    assert lib.sdfr_mesh_interpolate(fake, 3, 1, fake, 1, fake, fake, 2, 8, 8, fake, 3, 0.0,
                                     fake, None) == EINVAL
    assert b"background_batch" in lib.sdfr_last_error()
    assert lib.sdfr_mesh_interpolate(fake, 3, 0, fake, 1, fake, fake, 2, 8, 8, None, 0, 0.0,
                                     fake, None) == EINVAL
    assert b"zero size" in lib.sdfr_last_error()
    nul = None
    assert lib.sdfr_mesh_interpolate(nul, 3, 1, nul, 1, nul, nul, 1, 8, 8, nul, 0, 0.0, nul,
                                     nul) == EINVAL
    assert b"null attr" in lib.sdfr_last_error()


def test_noise_injection_without_projection_is_unchanged(sdfr):
    """The projecting layer leaves every other call as it was: fresh noise for noise=None,
    the given map without a transform."""
    ni = sdfr.NoiseInjection(project=True)
    with torch.no_grad():
        ni.weight.fill_(0.1)
    img = torch.zeros(1, 2, 8, 8)
    noise = torch.randn(1, 1, 8, 8)
    assert torch.equal(ni(img, noise=noise), img + ni.weight * noise)
    torch.manual_seed(1)
    a = ni(img, noise=None, transform=torch.eye(4)[None, :3], mesh_path="unused.obj")
    torch.manual_seed(1)
    assert torch.equal(a, img + ni.weight * torch.empty(1, 1, 8, 8).normal_())
    assert ni.prev_noise is None and ni.vert_noise is None
    assert sdfr.NoiseInjection.subdivisions(64) == 0 == sdfr.NoiseInjection.subdivisions(128)
    assert sdfr.NoiseInjection.subdivisions(256) == 1
    assert sdfr.NoiseInjection.subdivisions(512) == 3

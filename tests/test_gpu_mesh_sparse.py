"""GPU: narrow-band bricks and sparse marching cubes (csrc/mesh_sparse.hip,
mesh.sparse_extract / extract_mesh_sparse, Generator.extract_mesh) against the dense
marching cubes, the CPU oracle and the numpy model of tests/test_mesh_sparse.py.  Meshes
are compared in canonical form with assert_array_equal: the interpolation arithmetic and
the SDF values are the same bits on both sides."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests.golden import weights as W
from tests.test_fc_query import alive_inputs, alive_renderer
from tests.test_gpu_mesh import _closed_oriented_euler
from tests.test_gpu_render import DEV, make_renderer, make_siren
from tests.test_mesh_sparse import (assert_same_mesh, canonical, model_closure, model_layout,
                                    model_leaks, model_mesh)

pytestmark = pytest.mark.gpu

_record = {}


# ------------------------------------------------------------------------------- helpers
def _index_axes(res):
    a = torch.arange(res, dtype=torch.float32, device=DEV)
    return (a, a, a)


def _lookup(vol):
    """evaluate for index-valued axes: the dense volume at the points' indices."""
    def evaluate(p):
        i = p.long()
        return vol[i[:, 0], i[:, 1], i[:, 2]]
    return evaluate


def _sparse(sdfr, vol, seeds, level=0.0, grow=True):
    """sparse_extract on a dense GPU volume [res]^3 -> (verts, faces, SparseVolume), numpy."""
    res = vol.shape[0]
    s = torch.as_tensor(np.asarray(seeds, np.uint8)).to(DEV)
    v, f, sv = sdfr.sparse_extract(_lookup(vol), _index_axes(res), res, s, level, grow)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    return v.cpu().numpy(), f.cpu().numpy(), sv


def _dense(sdfr, vol, level=0.0):
    v, f = sdfr.marching_cubes(vol, level)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


def _no_unreferenced(v, f):
    np.testing.assert_array_equal(np.unique(f), np.arange(len(v)))


def _bricks(t, nb):
    return t.cpu().numpy().reshape(nb, nb, nb).astype(bool)


def _sphere(res, centre, radius):
    ax = torch.arange(res, device=DEV, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax - centre[0], ax - centre[1], ax - centre[2], indexing="ij")
    return torch.sqrt(x * x + y * y + z * z) - radius


# ------------------------------------------------------------------------- 1. all bricks
@pytest.mark.parametrize("res,level", [(16, 0.0), (24, 0.0), (16, 0.3)])
def test_all_bricks_stored_equals_dense(sdfr, res, level):
    """1. Random volumes with every brick a seed: brick-border edges, the cube's outer
    faces and every slot lookup; equal to the dense kernel, at 16^3 also to the oracle."""
    torch.manual_seed(res + int(level * 10))
    vol = torch.randn(res, res, res, device=DEV)
    nb = res // 8
    v, f, sv = _sparse(sdfr, vol, np.ones(nb ** 3), level)
    assert sv.rounds == 1 and sv.n_bricks == nb ** 3 and sv.stored_fraction == 1.0
    assert not sv.grow.any() and sv.res == res and sv.level == level
    _no_unreferenced(v, f)
    dv, df = _dense(sdfr, vol, level)
    assert len(v) == len(dv) and len(f) == len(df)
    assert_same_mesh(canonical(v, f), canonical(dv, df))
    assert torch.equal(sv.dense(), vol)
    if res == 16:
        from oracle import mc
        assert_same_mesh(canonical(v, f), canonical(*mc.marching_cubes(vol.cpu().numpy(), level)))


# ----------------------------------------------------------------------------- 2. layout
def _layout(sdfr, surface, slots, n_prev):
    lib = sdfr._lib.lib()
    nb = surface.shape[0]
    s = torch.from_numpy(surface.astype(np.uint8).ravel()).to(DEV)
    nbytes = lib.sdfr_brick_layout_workspace_bytes(nb)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    total = ctypes.c_uint32(0)
    sdfr._lib.check(lib.sdfr_brick_layout(sdfr._lib.ptr(s), nb, sdfr._lib.ptr(slots), n_prev,
                                          sdfr._lib.ptr(ws), nbytes, total,
                                          sdfr._lib.stream_of(slots)), "layout")
    return int(total.value)


def _hand_surface():
    s = np.zeros((5, 5, 5), bool)
    for k in ((0, 0, 0), (4, 4, 4), (2, 2, 0), (4, 1, 2), (1, 3, 3), (1, 3, 4), (0, 4, 2)):
        s[k] = True                         # corners, face bricks, two neighbours
    return s


def test_layout_matches_model_and_appends(sdfr):
    """2. res 40 (nb 5): slots and the total equal the model; a second call with n_prev
    keeps the old slots and appends the new ones in ascending q."""
    s = _hand_surface()
    slots = torch.full((125,), -1, dtype=torch.int32, device=DEV)
    n = _layout(sdfr, s, slots, 0)
    want, n_want = model_layout(s)
    assert n == n_want and 7 < n < 125
    np.testing.assert_array_equal(slots.cpu().numpy(), want)
    first = slots.cpu().numpy().copy()
    s2 = s.copy()
    s2[3, 0, 0] = s2[2, 2, 1] = s2[0, 0, 1] = True
    n2 = _layout(sdfr, s2, slots, n)
    want2, n2_want = model_layout(s2, want, n)
    got2 = slots.cpu().numpy()
    assert n2 == n2_want and n2 > n
    np.testing.assert_array_equal(got2, want2)
    np.testing.assert_array_equal(got2[first >= 0], first[first >= 0])
    added = np.flatnonzero((first < 0) & (got2 >= 0))
    np.testing.assert_array_equal(got2[added], n + np.arange(len(added)))
    assert _layout(sdfr, s2, slots, n2) == n2                      # nothing new: unchanged
    np.testing.assert_array_equal(slots.cpu().numpy(), want2)


# ----------------------------------------------------------------------------- 3. points
@pytest.mark.parametrize("res", [24, 40])
def test_brick_points_are_cube_points(sdfr, res):
    """3. With the cube's axes the points of the stored bricks are cube_points(res) at the
    stored indices bit for bit (2 / res is no power of two), in two slot ranges; NaN first."""
    lib = sdfr._lib.lib()
    nb = res // 8
    s = _hand_surface()[:nb, :nb, :nb]
    slots = torch.full((nb ** 3,), -1, dtype=torch.int32, device=DEV)
    n = _layout(sdfr, s, slots, 0)
    assert 2 <= n
    c = sdfr.cube_axis(res, DEV)
    axes = [c, -c, -c]
    cut = n // 2
    parts = []
    for s0, s1 in ((0, cut), (cut, n)):
        p = torch.full(((s1 - s0) * 512, 3), float("nan"), device=DEV)
        sdfr._lib.check(lib.sdfr_brick_points(sdfr._lib.ptr(slots), nb, s0, s1,
                                              *(sdfr._lib.ptr(a) for a in axes),
                                              sdfr._lib.ptr(p), sdfr._lib.stream_of(p)), "points")
        parts.append(p)
    got = torch.cat(parts).cpu().numpy().reshape(n, 8, 8, 8, 3)
    assert not np.isnan(got).any()
    cube = sdfr.cube_points(res, DEV).cpu().numpy()                 # [iy, ix, iz, 3]
    sl = slots.cpu().numpy()
    for q in np.flatnonzero(sl >= 0):
        bx, by, bz = q // (nb * nb), (q // nb) % nb, q % nb
        want = cube[8 * by:8 * by + 8, 8 * bx:8 * bx + 8, 8 * bz:8 * bz + 8].transpose(1, 0, 2, 3)
        np.testing.assert_array_equal(got[sl[q]], want)


# ---------------------------------------------------------------------- 4-6. sphere cases
RES, RADIUS = 64, 20.5
# Off-lattice and towards the cube's high corner: K + {0,1}^3 is clipped there, and the
# model stores 209 of the 512 bricks (142 seeds).  For a centre near the middle of the cube
# the same band stores 282: the seeds stay below a third, their dilation does not stay
# below half at this res.
CENTRE = (39.3, 40.1, 38.7)


@pytest.fixture(scope="module")
def sphere(sdfr):
    vol = _sphere(RES, CENTRE, RADIUS)
    mid = np.arange(RES // 8) * 8 + 4.0
    x, y, z = np.meshgrid(*(mid - c for c in CENTRE), indexing="ij")
    band = np.abs(np.sqrt(x * x + y * y + z * z) - RADIUS) <= 4 * np.sqrt(3)    # L = 1
    dense = _dense(sdfr, vol)
    return dict(vol=vol, np=vol.cpu().numpy(), band=band, dense=dense,
                canon=canonical(*dense))


def test_sphere_band_seeds(sdfr, sphere):
    """4. Exact band seeds (L = 1 in index units): the dense mesh in one round."""
    v, f, sv = _sparse(sdfr, sphere["vol"], sphere["band"])
    assert_same_mesh(canonical(v, f), sphere["canon"])
    _no_unreferenced(v, f)
    assert _closed_oriented_euler(v, f) == 2
    assert sv.rounds == 1 and not sv.grow.any()
    want, n_want = model_layout(sphere["band"])
    np.testing.assert_array_equal(sv.slots.cpu().numpy(), want)
    print(f"sphere: {int(sphere['band'].sum())} seeds, {sv.n_bricks} of 512 bricks stored")
    assert sv.n_bricks == n_want < 256 and sv.stored_fraction == n_want / 512
    stored = sv.slots.cpu().numpy().reshape(8, 8, 8) >= 0
    d = sv.dense().cpu().numpy()
    keep = np.repeat(np.repeat(np.repeat(stored, 8, 0), 8, 1), 8, 2)
    np.testing.assert_array_equal(d[keep], sphere["np"][keep])
    assert np.isnan(d[~keep]).all()


def _one_seed():
    seed = np.zeros((8, 8, 8), bool)
    seed[int(CENTRE[0] + RADIUS) // 8, int(CENTRE[1]) // 8, int(CENTRE[2]) // 8] = True
    return seed


def test_sphere_grows_from_one_brick(sdfr, sphere):
    """5. One seed brick on the surface: growth ends with case 4's mesh and the model's
    closure; without growth the first round's leaks and the model's partial mesh."""
    seed = _one_seed()
    v, f, sv = _sparse(sdfr, sphere["vol"], seed)
    assert_same_mesh(canonical(v, f), sphere["canon"])
    _no_unreferenced(v, f)
    closed, rounds = model_closure(sphere["np"], 0.0, seed)
    np.testing.assert_array_equal(_bricks(sv.surface, 8), closed)
    np.testing.assert_array_equal(_bricks(sv.seeds, 8), seed)
    assert sv.rounds == rounds > 1 and not sv.grow.any()
    assert (sv.slots.cpu().numpy() >= 0).sum() == sv.n_bricks == model_layout(closed)[1]
    v, f, sv = _sparse(sdfr, sphere["vol"], seed, grow=False)
    np.testing.assert_array_equal(_bricks(sv.grow, 8), model_leaks(sphere["np"], 0.0, seed))
    np.testing.assert_array_equal(_bricks(sv.surface, 8), seed)
    assert sv.grow.any() and sv.rounds == 1 and sv.n_bricks == model_layout(seed)[1]
    part = model_mesh(sphere["np"], 0.0, seed, sphere["dense"])
    assert 0 < len(part[1]) < len(sphere["canon"][1])
    assert_same_mesh(canonical(v, f), part)
    _no_unreferenced(v, f)


def test_two_spheres_one_unseeded(sdfr):
    """6. Growth follows the seeded component only: the model's mesh, a closed sphere."""
    c1, r1, c2, r2 = (20.3, 21.1, 19.7), 10.5, (45.2, 44.6, 46.1), 9.5
    vol = torch.minimum(_sphere(RES, c1, r1), _sphere(RES, c2, r2))
    seed = np.zeros((8, 8, 8), bool)
    seed[int(c1[0] + r1) // 8, int(c1[1]) // 8, int(c1[2]) // 8] = True
    v, f, sv = _sparse(sdfr, vol, seed)
    vn = vol.cpu().numpy()
    closed, rounds = model_closure(vn, 0.0, seed)
    np.testing.assert_array_equal(_bricks(sv.surface, 8), closed)
    assert sv.rounds == rounds
    dense = _dense(sdfr, vol)
    assert_same_mesh(canonical(v, f), model_mesh(vn, 0.0, closed, dense))
    assert 0 < len(f) < len(dense[1])
    assert _closed_oriented_euler(v, f) == 2
    assert np.abs(np.linalg.norm(v - np.float32(c1), axis=1) - r1).max() < 0.05
    one = _dense(sdfr, _sphere(RES, c1, r1))
    assert_same_mesh(canonical(v, f), canonical(*one))


def test_no_crossing_raises(sdfr):
    vol = torch.ones(16, 16, 16, device=DEV)
    with pytest.raises(ValueError):
        _sparse(sdfr, vol, np.ones(8))
    with pytest.raises(ValueError):
        _sparse(sdfr, vol, np.zeros(8))


# ------------------------------------------------------------------------------ 7. fields
FIELD_RES = 48


def _ngp(sdfr, golden_dir):
    sd = W.det_state_dict(W.golden_entries(golden_dir), "renderer.")
    lat = torch.from_numpy(np.load(golden_dir / "render_small.npz")["latent"]).to(DEV)
    return make_renderer(sdfr, sd, 8, 24, return_sdf=True), lat[:1]


def _siren(sdfr, golden_dir):
    sd = W.det_state_dict(W.golden_entries(golden_dir, siren=True), "renderer.")
    lat = torch.from_numpy(np.load(golden_dir / "render_siren_small.npz")["latent"]).to(DEV)
    return make_siren(sdfr, sd, 8, 24, return_sdf=True), lat[:1]


def _fc(sdfr, golden_dir):
    """tests/test_gpu_fc_query.py test 8: the alive set, sigma_linear's bias moved to put
    the cube's median SDF at zero."""
    ren = copy.deepcopy(alive_renderer(sdfr)).to(DEV)
    lat = alive_inputs()[1][:1].to(DEV)
    cp = sdfr.cube_points(FIELD_RES, DEV).reshape(1, -1, 3)
    with torch.no_grad():
        ren.network.sigma_linear.bias -= ren.query(cp, lat, return_rgb=False)[0].median()
    return ren, lat


FIELDS = {"ngp": _ngp, "siren": _siren, "fc": _fc}


def _field_case(sdfr, ren, lat, **kw):
    """extract_mesh_sparse against the model on sdf_cube's dense volume with the call's own
    seeds -> (mesh, share of the dense triangles left out)."""
    res, nb = FIELD_RES, FIELD_RES // 8
    mesh, sv = sdfr.extract_mesh_sparse(ren, lat, res=res, return_volume=True, **kw)
    with torch.no_grad():
        cube = sdfr.sdf_cube(ren, lat, res=res)
    full = sdfr.extract_mesh_with_marching_cubes(cube)
    vol = cube[0, ..., 0].permute(1, 0, 2)                           # (ix, iy, iz)
    vn = vol.cpu().numpy()
    stored = np.repeat(np.repeat(np.repeat(_bricks(sv.slots >= 0, nb), 8, 0), 8, 1), 8, 2)
    np.testing.assert_array_equal(sv.dense().cpu().numpy()[stored], vn[stored])
    closed, rounds = model_closure(vn, 0.0, _bricks(sv.seeds, nb))
    np.testing.assert_array_equal(_bricks(sv.surface, nb), closed)
    assert sv.rounds == rounds
    want = model_mesh(vn, 0.0, closed, (full.vertices, full.faces))   # (dense cell order)
    assert mesh.vertices.dtype == np.float32 and mesh.faces.dtype == np.int64
    assert_same_mesh(canonical(mesh.vertices, mesh.faces), want)
    _no_unreferenced(mesh.vertices, mesh.faces)
    return mesh, sv, 1.0 - len(mesh.faces) / len(full.faces)


@pytest.mark.parametrize("kind", ["ngp", "siren", "fc"])
def test_field_mesh_equals_model_on_dense_cube(sdfr, golden_dir, kind):
    """7. The three networks on the sdf_cube tests' renderers and latents at res 48, sampled
    L.  The op-by-op networks on the CPU give every one of the 216 bricks as a seed for the
    SIREN (L 3.85) and FC (alive set, L 21.4) fixtures, so nothing may be left out there."""
    ren, lat = FIELDS[kind](sdfr, golden_dir)
    mesh, sv, left_out = _field_case(sdfr, ren, lat)
    _record[kind] = dict(left_out=left_out, stored_fraction=sv.stored_fraction,
                         rounds=sv.rounds, faces=len(mesh.faces))
    print(f"{kind}: left out {left_out:.4f} of the dense triangles, stored "
          f"{sv.stored_fraction:.3f}, rounds {sv.rounds}, {len(mesh.faces)} triangles")
    assert len(mesh.faces) > 0
    if kind != "ngp":
        assert left_out == 0
    V = len(mesh.vertices)
    col = sdfr.color_mesh(mesh, ren, lat)
    assert col.shape == (V, 3) and col.min() >= 0.0 and col.max() <= 1.0
    n = sdfr.normal_mesh(mesh, ren, lat)
    assert n.shape == (V, 3) and np.isfinite(n).all()


def test_fixed_lipschitz_and_no_growth(sdfr, golden_dir):
    """7b. A small fixed L on the SIREN fixture seeds fewer bricks; the result still equals
    the model (with growth: the closure; without: the seeds' cells)."""
    ren, lat = _siren(sdfr, golden_dir)
    _, sv, _ = _field_case(sdfr, ren, lat, lipschitz=0.05)
    nb3 = (FIELD_RES // 8) ** 3
    assert 0 < int(sv.seeds.sum()) < nb3
    mesh, sv = sdfr.extract_mesh_sparse(ren, lat, res=FIELD_RES, lipschitz=0.05, grow=False,
                                        return_volume=True)
    assert sv.rounds == 1 and torch.equal(sv.surface, sv.seeds)
    with torch.no_grad():
        vn = sdfr.sdf_cube(ren, lat, res=FIELD_RES)[0, ..., 0].permute(1, 0, 2).cpu().numpy()
    np.testing.assert_array_equal(_bricks(sv.grow, FIELD_RES // 8),
                                  model_leaks(vn, 0.0, _bricks(sv.seeds, FIELD_RES // 8)))


def test_generator_extract_mesh_is_the_renderer_call(sdfr):
    """7c. Generator.extract_mesh = forward's mapping network and truncation, then
    extract_mesh_sparse on the mapped latent."""
    opt = sdfr.vol_render_opt(ngp=False)
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    z = torch.randn(1, 256, device=DEV)
    mean = [torch.randn(1, 256, device=DEV) * 0.1]
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z], None, 0.7, mean, False)[0]
        level = float(sdfr.sdf_cube(g.renderer, lat, res=16).median())
        want = sdfr.extract_mesh_sparse(g.renderer, lat, res=32, level=level)
        got = g.extract_mesh([z], res=32, truncation=0.7, truncation_latent=mean, level=level)
    assert len(want.faces) > 0
    np.testing.assert_array_equal(got.vertices, want.vertices)
    np.testing.assert_array_equal(got.faces, want.faces)


# ------------------------------------------------------------------------- 8. determinism
def test_two_runs_are_identical_in_raw_order(sdfr, golden_dir):
    """8. Vertex and triangle order is a pure function of the slot table and the values."""
    ren, lat = _ngp(sdfr, golden_dir)
    a = sdfr.extract_mesh_sparse(ren, lat, res=FIELD_RES)
    b = sdfr.extract_mesh_sparse(ren, lat, res=FIELD_RES)
    np.testing.assert_array_equal(a.vertices, b.vertices)
    np.testing.assert_array_equal(a.faces, b.faces)

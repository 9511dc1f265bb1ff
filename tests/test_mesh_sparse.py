"""CPU: narrow-band bricks and sparse marching cubes (include/sdfr.h "Sparse marching
cubes", csrc/mesh_sparse.hip, mesh.sparse_extract / extract_mesh_sparse): cube_axis, the
argument checks of the Python calls and of the C ABI, and a small numpy MODEL of the
header's definitions -- layout order, leak rule, closure, and the part of the dense mesh
that a surface set keeps -- checked here on hand-made 16^3 cases and reused by
tests/test_gpu_mesh_sparse.py as the reference of the kernels."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch


# ------------------------------------------------------------------------------ the model
def model_layout(surface, slots=None, n_prev=0):
    """``surface`` [nb, nb, nb] bool -> (slots [nb^3] int32, n_total): the bricks of
    K + {0,1}^3 (clipped) of every surface brick K that have no slot get n_prev,
    n_prev + 1, ... in ascending q = (bx nb + by) nb + bz; existing slots stay."""
    surface = np.asarray(surface, bool)
    nb = surface.shape[0]
    needed = np.zeros_like(surface)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                needed[a:, b:, c:] |= surface[:nb - a, :nb - b, :nb - c]
    slots = np.full(nb ** 3, -1, np.int32) if slots is None else np.array(slots, np.int32)
    new = needed.ravel() & (slots < 0)
    slots[new] = n_prev + np.arange(int(new.sum()), dtype=np.int32)
    return slots, n_prev + int(new.sum())


def model_leaks(vol, level, surface):
    """grow [nb, nb, nb] bool: brick K' (not surface) is set when a cell of a surface brick
    shares a face with a cell of K' and the face's four corners are not all on one side."""
    vol = np.asarray(vol, np.float32)
    surface = np.asarray(surface, bool)
    res, nb = vol.shape[0], surface.shape[0]
    inside = vol < np.float32(level)
    cb = np.arange(res - 1) >> 3                          # brick of a cell, per axis
    grow = np.zeros_like(surface)
    for d in range(3):
        ins, sf, gr = (np.moveaxis(x, d, 0) for x in (inside, surface, grow))
        for p in range(8, res - 1, 8):                    # the plane between cells p-1 and p
            s = ins[p].astype(np.int8)
            cnt = s[:-1, :-1] + s[1:, :-1] + s[:-1, 1:] + s[1:, 1:]
            mixed = (cnt > 0) & (cnt < 4)                 # [res-1, res-1] over the cells
            lo = sf[(p - 1) >> 3][np.ix_(cb, cb)]
            hi = sf[p >> 3][np.ix_(cb, cb)]
            for src, dst, b in ((lo, hi, p >> 3), (hi, lo, (p - 1) >> 3)):
                hit = np.zeros((nb, nb), np.int64)
                np.add.at(hit, (cb[:, None], cb[None, :]), (src & ~dst & mixed).astype(np.int64))
                gr[b] |= hit > 0                          # (a view: writes through to grow)
    return grow


def model_closure(vol, level, seeds):
    """(surface [nb, nb, nb] bool, rounds): seeds closed under leaks; rounds counts the
    classify passes, the last one without a leak."""
    surface = np.array(seeds, bool)
    rounds = 1
    while True:
        g = model_leaks(vol, level, surface)
        if not g.any():
            return surface, rounds
        surface |= g
        rounds += 1


def canonical(verts, faces):
    """Vertices sorted lexicographically, faces remapped, each rotated to start at its
    smallest index, faces sorted."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    order = np.lexsort((verts[:, 2], verts[:, 1], verts[:, 0]))
    inv = np.empty(len(verts), np.int64)
    inv[order] = np.arange(len(verts))
    f = inv[faces]
    k = f.argmin(axis=1)
    f = np.take_along_axis(f, (k[:, None] + np.arange(3)) % 3, axis=1)
    f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]
    return verts[order], f


def model_mesh(vol, level, surface, dense=None):
    """Canonical form of the dense mesh's triangles whose cell lies in a surface brick, with
    the vertices they reference.  ``dense`` = (verts, faces) of the dense marching cubes on
    ``vol`` in its own order (cell order); default: the CPU oracle's."""
    from oracle import mc
    vol = np.asarray(vol, np.float32)
    surface = np.asarray(surface, bool)
    res = vol.shape[0]
    v, f = mc.marching_cubes(vol, level) if dense is None else dense
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
    _, ntri = mc.table()
    inside = vol < np.float32(level)
    case = np.zeros((res - 1,) * 3, np.int64)
    for c in range(8):
        x, y, z = c & 1, (c >> 1) & 1, c >> 2
        case |= inside[x:res - 1 + x, y:res - 1 + y, z:res - 1 + z].astype(np.int64) << c
    nt = ntri[case].astype(np.int64)
    assert nt.sum() == len(f)
    cb = np.arange(res - 1) >> 3
    keep = np.repeat(surface[np.ix_(cb, cb, cb)].ravel(), nt.ravel())
    f = f[keep]
    used = np.unique(f)
    remap = np.full(len(v), -1, np.int64)
    remap[used] = np.arange(len(used))
    return canonical(v[used], remap[f])


def assert_same_mesh(got, want):
    """Both in canonical form, bit for bit."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


# -------------------------------------------------------------- the model on hand-made cases
def _plane16():
    """16^3, value ix - 7.5: the surface is the plane x = 7.5, inside the cells with low
    corner ix = 7, which belong to the four bricks bx = 0."""
    return np.broadcast_to((np.arange(16, dtype=np.float32) - 7.5)[:, None, None],
                           (16, 16, 16)).copy()


def test_model_layout_order_by_hand():
    s = np.zeros((2, 2, 2), bool)
    s[1, 1, 1] = True                       # its {0,1}^3 neighbours are clipped away
    slots, n = model_layout(s)
    assert n == 1 and slots.tolist() == [-1] * 7 + [0]
    s[0, 0, 0] = True                       # now all eight; the old slot stays
    slots, n = model_layout(s, slots, n)
    assert n == 8 and slots.tolist() == [1, 2, 3, 4, 5, 6, 7, 0]
    s = np.zeros((3, 3, 3), bool)
    s[1, 0, 2] = True                       # K + {0,1}^3 clipped at bz = 2
    slots, n = model_layout(s)
    want = np.full(27, -1)
    want[[(1 * 3 + 0) * 3 + 2, (1 * 3 + 1) * 3 + 2, (2 * 3 + 0) * 3 + 2, (2 * 3 + 1) * 3 + 2]] = \
        [0, 1, 2, 3]
    assert n == 4 and slots.tolist() == want.tolist()


def test_model_leaks_closure_and_mesh_by_hand():
    vol = _plane16()
    seed = np.zeros((2, 2, 2), bool)
    seed[0, 0, 0] = True
    g = model_leaks(vol, 0.0, seed)
    want = np.zeros((2, 2, 2), bool)
    want[0, 1, 0] = want[0, 0, 1] = True    # across +y and +z; the +x face (x = 8) is all outside
    np.testing.assert_array_equal(g, want)
    surface, rounds = model_closure(vol, 0.0, seed)
    want[0, 0, 0] = want[0, 1, 1] = True
    np.testing.assert_array_equal(surface, want)
    assert rounds == 3                      # (0,0,0) -> two neighbours -> (0,1,1) -> none
    # the seed brick alone: 8 x 8 cells of two triangles on 9 x 9 vertices at x = 7.5
    v, f = model_mesh(vol, 0.0, seed)
    assert v.shape == (81, 3) and f.shape == (128, 3)
    assert np.all(v[:, 0] == 7.5) and v[:, 1:].max() == 8 and len(np.unique(f)) == 81
    # the closure: the whole plane, equal to the dense mesh
    from oracle import mc
    v, f = model_mesh(vol, 0.0, surface)
    assert v.shape == (256, 3) and f.shape == (450, 3)
    assert_same_mesh((v, f), canonical(*mc.marching_cubes(vol, 0.0)))
    # a seed off the surface's bricks closes to itself and keeps nothing
    off = np.zeros((2, 2, 2), bool)
    off[1, 0, 0] = True
    surface, rounds = model_closure(vol, 0.0, off)
    np.testing.assert_array_equal(surface, off)
    assert rounds == 1 and len(model_mesh(vol, 0.0, off)[1]) == 0


def test_canonical_form_forgets_order():
    v = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]])
    f = np.array([[0, 1, 2], [3, 1, 0]])
    perm = np.array([2, 0, 3, 1])           # new vertex i is old vertex perm[i]
    inv = np.argsort(perm)
    f2 = np.roll(inv[f], 1, axis=1)[::-1]
    assert_same_mesh(canonical(v[perm], f2), canonical(v, f))


# ------------------------------------------------------------------------- the Python calls
def test_cube_axis_is_cube_points_axes(sdfr):
    for res in (8, 24, 40, 48, 100):        # 2 / res is not a power of two for most
        c = sdfr.cube_axis(res)
        assert c.shape == (res,) and c.dtype == torch.float32
        assert torch.equal(c, torch.arange(res, dtype=torch.float32) * 2 / res - 1)
        p = sdfr.cube_points(res)           # [iy, ix, iz] -> (c(ix), -c(iy), -c(iz))
        assert torch.equal(p[0, :, 0, 0], c)
        assert torch.equal(p[:, 0, 0, 1], -c) and torch.equal(p[0, 0, :, 2], -c)
        assert torch.equal(p[..., 0], c.view(1, res, 1).expand(res, res, res))


def _never(points):
    raise AssertionError("evaluate must not be reached")


@pytest.mark.parametrize("res", [8, 12, 20, 36, 0, 2056])
def test_bad_res_is_a_value_error(sdfr, res):
    axes = (torch.zeros(max(res, 1)),) * 3
    with pytest.raises(ValueError, match="res"):
        sdfr.sparse_extract(_never, axes, res, torch.ones(max(res // 8, 1) ** 3))
    with pytest.raises(ValueError, match="res"):
        sdfr.extract_mesh_sparse(None, torch.zeros(1, 256), res=res)


def test_cpu_tensors_and_bad_shapes(sdfr):
    axes = (torch.zeros(16),) * 3
    with pytest.raises(RuntimeError, match="GPU"):
        sdfr.sparse_extract(_never, axes, 16, torch.ones(8))
    with pytest.raises(RuntimeError, match="GPU"):
        sdfr.extract_mesh_sparse(None, torch.zeros(1, 256), res=16)
    with pytest.raises(ValueError, match="seeds"):
        sdfr.sparse_extract(_never, axes, 16, torch.ones(9))
    with pytest.raises(ValueError, match="axes"):
        sdfr.sparse_extract(_never, (torch.zeros(16), torch.zeros(16), torch.zeros(15)), 16,
                            torch.ones(8))
    with pytest.raises(ValueError, match="one face"):
        sdfr.extract_mesh_sparse(None, torch.zeros(2, 256), res=16)


# ------------------------------------------------------------------------------ the C ABI
def _rejected(sdfr, rc, msg):
    lib = sdfr._lib.lib()
    assert rc == sdfr._lib.SDFR_EINVAL
    assert msg in lib.sdfr_last_error(), lib.sdfr_last_error()


def test_c_abi_rejects_bad_arguments_before_any_launch(sdfr):
    """Every SDFR_EINVAL case of the header on fake pointers: nothing is launched."""
    lib = sdfr._lib.lib()
    u32 = ctypes.c_uint32
    out, counts = u32(0), (u32 * 2)()
    # layout
    lay = lib.sdfr_brick_layout_workspace_bytes
    assert lay(2) >= 9 * 4 and lay(256) >= (256 ** 3 + 1) * 4 and lay(0) == 0 == lay(257)
    good = [FAKE, 2, FAKE, 0, FAKE, lay(2), out, None]
    for i in (0, 2, 4, 6):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_brick_layout(*a), b"brick_layout: null")
    for nb in (0, 257):
        a = list(good)
        a[1], a[5] = nb, 1 << 40
        _rejected(sdfr, lib.sdfr_brick_layout(*a), b"nb must be in [1, 256]")
    a = list(good)
    a[5] -= 1
    _rejected(sdfr, lib.sdfr_brick_layout(*a), b"workspace too small")
    # points
    good = [FAKE, 2, 0, 3, FAKE, FAKE, FAKE, FAKE, None]
    for i in (0, 4, 5, 6, 7):
        a = list(good)
        a[i] = None
        _rejected(sdfr, lib.sdfr_brick_points(*a), b"brick_points: null")
    for nb in (0, 257):
        a = list(good)
        a[1] = nb
        _rejected(sdfr, lib.sdfr_brick_points(*a), b"nb must be in [1, 256]")
    for s0, s1 in ((3, 3), (4, 3), (0, 0)):
        a = list(good)
        a[2], a[3] = s0, s1
        _rejected(sdfr, lib.sdfr_brick_points(*a), b"empty slot range")
    # count / emit
    size = lib.sdfr_mc_sparse_workspace_bytes
    n_max = (1 << 21) - 1                   # 4 * 512 n + 1 < 2^32
    assert size(0) == 0 == size(n_max + 1) and size(1 << 31) == 0
    assert size(1) >= (4 * 512 + 1) * 4 + 4 and size(n_max) >= 16 * 512 * n_max
    assert size(9) - size(8) >= 16 * 512
    head = [FAKE, FAKE, FAKE, 2, 8, 0.0, FAKE, size(8)]
    calls = ((lib.sdfr_mc_sparse_count, [None, counts, None], b"null counts", (1,)),
             (lib.sdfr_mc_sparse_emit, [FAKE, FAKE, None], b"null verts / faces", (0, 1)))
    for fn, tail, tail_msg, tail_ptrs in calls:
        for i in (0, 1, 2, 6):
            a = list(head)
            a[i] = None
            _rejected(sdfr, fn(*a, *tail), b"mc_sparse: null values")
        for i in tail_ptrs:
            t = list(tail)
            t[i] = None
            _rejected(sdfr, fn(*head, *t), tail_msg)
        for nb in (0, 257):
            a = list(head)
            a[3] = nb
            _rejected(sdfr, fn(*a, *tail), b"nb must be in [1, 256]")
        a = list(head)
        a[4] = 0
        _rejected(sdfr, fn(*a, *tail), b"no bricks")
        for n in (n_max + 1, (1 << 32) - 1):
            a = list(head)
            a[4], a[7] = n, (1 << 64) - 1
            _rejected(sdfr, fn(*a, *tail), b"too many bricks")
        a = list(head)
        a[4], a[7] = n_max, 0               # the largest count passes on to the size check
        _rejected(sdfr, fn(*a, *tail), b"workspace too small")
        a = list(head)
        a[7] -= 1
        _rejected(sdfr, fn(*a, *tail), b"workspace too small")

"""CPU: the field query's C-ABI argument checks and workspace size
(sdfr_query_ngp_forward, include/sdfr.h ABI 14), the cube / colour helpers of
mesh.py, and VolumeFeatureRenderer.query's op-by-op path."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 0x1000          # a non-null pointer value: rejections happen before any launch


def _weights(sdfr):
    """sdfr_ngp_weights with every pointer non-null (never dereferenced on the host)."""
    w = sdfr._lib.NgpWeights()
    for name, typ in w._fields_:
        if typ is ctypes.c_void_p:
            setattr(w, name, FAKE)
        elif typ not in (ctypes.c_uint32, ctypes.c_float):
            setattr(w, name, typ(*([FAKE] * 3)))
    w.num_levels, w.base_resolution, w.bound = 16, 16, 2.0
    return w


def _args(sdfr, B=1, R=16, N=32):
    lib = sdfr._lib.lib()
    return sdfr._lib.NgpQueryArgs(
        B=B, R=R, N=N, points=FAKE, dirs=FAKE, styles=FAKE, sdf=FAKE, rgb=None, workspace=FAKE,
        workspace_bytes=lib.sdfr_query_ngp_workspace_bytes(B, R, N), prepacked=None)


def _rejected(sdfr, w, a, msg):
    lib = sdfr._lib.lib()
    rc = lib.sdfr_query_ngp_forward(None if w is None else ctypes.byref(w),
                                    None if a is None else ctypes.byref(a), None)
    assert rc == sdfr._lib.SDFR_EINVAL
    assert msg in lib.sdfr_last_error(), lib.sdfr_last_error()


def test_query_rejects_bad_arguments_before_any_launch(sdfr):
    w = _weights(sdfr)
    _rejected(sdfr, None, _args(sdfr), b"null args")
    _rejected(sdfr, w, None, b"null args")
    for zero in ("B", "R", "N"):
        a = _args(sdfr)
        setattr(a, zero, 0)
        _rejected(sdfr, w, a, b"empty batch / group / point count")
    for field in ("points", "dirs", "styles", "sdf", "workspace"):
        a = _args(sdfr)
        setattr(a, field, None)
        _rejected(sdfr, w, a, b"required pointer is null")
    w2 = _weights(sdfr)
    w2.sigma_w = None
    _rejected(sdfr, w2, _args(sdfr), b"weight pointer is null")
    a = _args(sdfr)
    a.workspace_bytes -= 1
    _rejected(sdfr, w, a, b"workspace too small")
    a.workspace_bytes = 0
    _rejected(sdfr, w, a, b"workspace too small")
    # 2^25 padded points: one more 16-group tile than a call may hold
    a = _args(sdfr, B=1, R=1 << 20, N=32)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, w, a, b"too many samples per call")
    a = _args(sdfr, B=1 << 20, R=1 << 20, N=1 << 20)
    a.workspace_bytes = (1 << 64) - 1
    _rejected(sdfr, w, a, b"too many samples per call")


def test_query_workspace_grows_with_padded_points(sdfr):
    """144 bytes per point of the padded count S = B ceil(R/16) 16 N: its 16 x 2 gathered
    features (128 B) and its grid coordinate + inside flag (16 B)."""
    ws = sdfr._lib.lib().sdfr_query_ngp_workspace_bytes
    base = ws(1, 16, 32)
    assert base >= 144 * 16 * 32
    assert ws(1, 1, 32) == base == ws(1, 15, 32)                 # one padded tile
    assert ws(1, 17, 32) == ws(1, 32, 32) == base + 144 * 16 * 32
    assert ws(1, 16, 33) == base + 144 * 16
    assert ws(1, 4096, 32) == base + 144 * (4096 - 16) * 32
    # a second face: its points and its FiLM vectors (4 layers x (gamma, beta) x 256)
    assert ws(2, 16, 32) == base + 144 * 16 * 32 + 4 * 2 * 256 * 4


def test_cube_points_match_marching_cubes_vertex_scaling(sdfr):
    """Index (iy, ix, iz) of cube_points holds the network coordinate of the world
    position extract_mesh_with_marching_cubes assigns to index (ix, iy, iz):
    (i / res - 0.5) * 0.24 per axis with y and z negated, times 2 / (far - near)."""
    res = 4
    p = sdfr.cube_points(res)
    assert p.shape == (res, res, res, 3) and p.dtype == torch.float32
    c = [2 * i / res - 1 for i in range(res)]                    # exact in fp32 at res = 4
    for iy in range(res):
        for ix in range(res):
            for iz in range(res):
                assert p[iy, ix, iz].tolist() == [c[ix], -c[iy], -c[iz]]
                world = np.array([(ix / res - 0.5) * 0.24, -(iy / res - 0.5) * 0.24,
                                  -(iz / res - 0.5) * 0.24])
                np.testing.assert_allclose(sdfr.world_to_network(world), p[iy, ix, iz].numpy(),
                                           rtol=0, atol=1e-12)
    assert sdfr.world_to_network(0.12, 0.88, 1.12) == pytest.approx(1.0)


def test_mesh_export_with_and_without_vertex_colors(sdfr, tmp_path):
    v = [[0.0, 0.5, -1.0], [1.0, 0.25, 0.125], [-0.5, 2.0, 3.0]]
    m = sdfr.Mesh(v, [[0, 1, 2]])
    plain = ("v 0.00000000 0.50000000 -1.00000000\n"
             "v 1.00000000 0.25000000 0.12500000\n"
             "v -0.50000000 2.00000000 3.00000000\n"
             "f 1 2 3\n")
    assert m.vertex_colors is None
    assert m.export(file_type="obj") == plain
    m.vertex_colors = np.array([[0, 0.5, 1], [0.25, 0.125, 0.75], [1, 1, 0]], np.float32)
    colored = ("v 0.00000000 0.50000000 -1.00000000 0.000000 0.500000 1.000000\n"
               "v 1.00000000 0.25000000 0.12500000 0.250000 0.125000 0.750000\n"
               "v -0.50000000 2.00000000 3.00000000 1.000000 1.000000 0.000000\n"
               "f 1 2 3\n")
    path = tmp_path / "m.obj"
    assert m.export(str(path)) == colored
    assert path.read_text() == colored
    m.vertex_colors = None
    assert m.export() == plain
    m.vertex_colors = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="vertex_colors"):
        m.export()


def test_query_module_path_equals_network_slices(sdfr):
    """Off the fused path (here: an FC renderer on CPU tensors) query is
    renderer.network on cat([points, dirs]), sliced: sdf = channel 3, rgb =
    sigmoid(channels 0..2), for all three viewdirs forms."""
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    torch.manual_seed(3)
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=8).eval()
    B, M = 2, 5
    pts = torch.rand(B, M, 3) * 2 - 1
    lat = torch.randn(B, 256)
    d_face = torch.nn.functional.normalize(torch.randn(B, 3), dim=-1)
    d_point = torch.nn.functional.normalize(torch.randn(B, M, 3), dim=-1)
    with torch.no_grad():
        for vd, full in ((d_face, d_face[:, None].expand(B, M, 3)), (d_point, d_point)):
            raw = ren.network(torch.cat([pts, full], -1), styles=lat)
            sdf, rgb = ren.query(pts, lat, viewdirs=vd)
            assert sdf.shape == (B, M) and rgb.shape == (B, M, 3)
            assert torch.equal(sdf, raw[..., 3])
            assert torch.equal(rgb, torch.sigmoid(raw[..., :3]))
            sdf2, none = ren.query(pts, lat, viewdirs=vd, return_rgb=False)
            assert none is None and torch.equal(sdf2, sdf)
        raw = ren.network(torch.cat([pts, torch.zeros(B, M, 3)], -1), styles=lat)
        sdf, none = ren.query(pts, lat, return_rgb=False)
        assert none is None and sdf.shape == (B, M) and torch.equal(sdf, raw[..., 3])
    with pytest.raises(ValueError, match="viewdirs"):
        ren.query(pts, lat)                                   # rgb needs a direction
    with pytest.raises(ValueError, match="viewdirs"):
        ren.query(pts, lat, viewdirs=torch.zeros(B, M + 1, 3))
    with pytest.raises(ValueError, match="points"):
        ren.query(pts[0], lat, viewdirs=d_face)
    # under grad the call stays on the autograd path and is differentiable
    p = pts.clone().requires_grad_(True)
    sdf, _ = ren.query(p, lat, viewdirs=d_face)
    sdf.sum().backward()
    assert p.grad is not None and p.grad.shape == p.shape


"""CPU: the SDF-gradient query's C-ABI argument checks and workspace size
(sdfr_query_ngp_grad, include/sdfr.h ABI 15), VolumeFeatureRenderer.query_gradient's
autograd path, and the normal / eikonal helpers of mesh.py."""
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


def _args(sdfr, B=1, M=40):
    lib = sdfr._lib.lib()
    return sdfr._lib.NgpGradArgs(
        B=B, M=M, points=FAKE, styles=FAKE, sdf=None, grad=FAKE, workspace=FAKE,
        workspace_bytes=lib.sdfr_query_ngp_grad_workspace_bytes(B, M), prepacked=None)


def _rejected(sdfr, w, a, msg, code=None):
    lib = sdfr._lib.lib()
    rc = lib.sdfr_query_ngp_grad(None if w is None else ctypes.byref(w),
                                 None if a is None else ctypes.byref(a), None)
    assert rc == (sdfr._lib.SDFR_EINVAL if code is None else code)
    assert msg in lib.sdfr_last_error(), lib.sdfr_last_error()


def test_abi_version_is_15(sdfr):
    assert sdfr._lib.ABI_VERSION == 15 == sdfr._lib.lib().sdfr_abi_version()


def test_gradient_rejects_bad_arguments_before_any_launch(sdfr):
    w = _weights(sdfr)
    _rejected(sdfr, None, _args(sdfr), b"null args")
    _rejected(sdfr, w, None, b"null args")
    for zero in ("B", "M"):
        a = _args(sdfr)
        setattr(a, zero, 0)
        _rejected(sdfr, w, a, b"empty batch / point count")
    for field in ("points", "styles", "grad", "workspace"):
        a = _args(sdfr)
        setattr(a, field, None)
        _rejected(sdfr, w, a, b"required pointer is null")
    w2 = _weights(sdfr)
    w2.sigma_w = None
    _rejected(sdfr, w2, _args(sdfr), b"weight pointer is null")
    w2 = _weights(sdfr)
    w2.pts_gw = (ctypes.c_void_p * 3)(FAKE, None, FAKE)
    _rejected(sdfr, w2, _args(sdfr), b"FiLM weight pointer is null")
    w2 = _weights(sdfr)
    w2.num_levels = 8
    _rejected(sdfr, w2, _args(sdfr), b"needs 16 levels", sdfr._lib.SDFR_EUNSUPPORTED)
    a = _args(sdfr)
    a.workspace_bytes -= 1
    _rejected(sdfr, w, a, b"workspace too small")
    a.workspace_bytes = 0
    _rejected(sdfr, w, a, b"workspace too small")
    # The kernels index the gather's output in fp32 elements, 128 per padded point, with
    # 32-bit arithmetic: 2^25 padded points (M rounded up to 8 per face) are the first
    # rejected size; one padding unit below passes that check and reaches the next one.
    a = _args(sdfr, B=1, M=(1 << 25) - 7)
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, w, a, b"too many points per call")
    a = _args(sdfr, B=1, M=(1 << 25) - 8)
    a.workspace_bytes = 0
    _rejected(sdfr, w, a, b"workspace too small")
    a = _args(sdfr, B=4, M=(1 << 23))
    a.workspace_bytes = 1 << 62
    _rejected(sdfr, w, a, b"too many points per call")
    # sizes whose byte counts (B Mp x 128 elements, x 512 bytes) wrap in 64 bits
    for B, M in (((1 << 32) - 1, (1 << 32) - 1), (1 << 26, 1 << 31), (1 << 23, (1 << 32) - 1),
                 (1 << 31, 1 << 26)):
        a = _args(sdfr, B=B, M=M)
        a.workspace_bytes = (1 << 64) - 1
        _rejected(sdfr, w, a, b"too many points per call")
        a.workspace_bytes = 0
        _rejected(sdfr, w, a, b"too many points per call")


def test_gradient_workspace_grows_with_padded_points(sdfr):
    """512 bytes per padded point (M rounded up to 8 per face): its 32 gathered features
    and their 3 x 32 derivatives with respect to the grid coordinate."""
    ws = sdfr._lib.lib().sdfr_query_ngp_grad_workspace_bytes
    base = ws(1, 8)
    assert base >= 512 * 8
    assert ws(1, 1) == base == ws(1, 7)                          # one padded wave pass
    assert ws(1, 9) == ws(1, 16) == base + 512 * 8
    assert ws(1, 4096) == base + 512 * (4096 - 8)
    # a second face adds only its FiLM vectors (4 layers x (gamma, beta) x 256)
    assert ws(2, 2048) == ws(1, 4096) + 4 * 2 * 256 * 4
    assert ws(2, 8) == base + 512 * 8 + 4 * 2 * 256 * 4
    # a size one call cannot take has no workspace size
    assert ws(1, (1 << 25) - 8) == base + 512 * ((1 << 25) - 16)
    assert ws(1, (1 << 25) - 7) == 0 == ws(1 << 26, 1 << 31) == ws((1 << 32) - 1, (1 << 32) - 1)


def test_query_gradient_module_path_equals_autograd(sdfr):
    """Off the fused path (here: an FC renderer on CPU tensors) query_gradient is
    autograd.grad of the network's SDF sum with respect to the points, exactly; it works
    under no_grad and leaves the caller's tensor alone."""
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    torch.manual_seed(3)
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=8).eval()
    B, M = 2, 5
    pts = torch.rand(B, M, 3) * 2 - 1
    lat = torch.randn(B, 256)
    p = pts.clone().requires_grad_(True)
    raw = ren.network(torch.cat([p, torch.zeros(B, M, 3)], -1), styles=lat)
    want, = torch.autograd.grad(raw[..., 3].sum(), p)
    assert want.abs().max() > 0
    sdf, grad = ren.query_gradient(pts, lat)
    assert sdf.shape == (B, M) and grad.shape == (B, M, 3)
    assert torch.equal(grad, want) and torch.equal(sdf, raw[..., 3].detach())
    assert not sdf.requires_grad and not grad.requires_grad
    assert pts.grad is None and not pts.requires_grad
    with torch.no_grad():
        sdf2, grad2 = ren.query_gradient(pts, lat)
    assert torch.equal(grad2, want) and torch.equal(sdf2, sdf)
    # a caller's tensor that requires grad keeps its flag and gets no .grad
    q = pts.clone().requires_grad_(True)
    _, grad3 = ren.query_gradient(q, lat)
    assert torch.equal(grad3, want) and q.requires_grad and q.grad is None
    # normalize: unit rows; a zero gradient stays zero
    _, n = ren.query_gradient(pts, lat, normalize=True)
    torch.testing.assert_close(n.norm(dim=-1), torch.ones(B, M), rtol=0, atol=1e-6)
    torch.testing.assert_close(n, want / want.norm(dim=-1, keepdim=True), rtol=0, atol=1e-6)

    class _Flat(torch.nn.Module):
        """A network whose SDF ignores the points of face 1 (zero gradient there)."""
        def forward(self, x, styles):
            out = x[..., :1] * 3.0 * torch.tensor([1.0, 0.0]).view(2, 1, 1)
            return torch.cat([torch.zeros_like(x[..., :3]), out], -1)

    ren.network = _Flat()
    _, n = ren.query_gradient(pts, lat, normalize=True)
    assert torch.equal(n[0], torch.tensor([1.0, 0.0, 0.0]).expand(M, 3))
    assert torch.equal(n[1], torch.zeros(M, 3))
    with pytest.raises(ValueError, match="points"):
        ren.query_gradient(pts[0], lat)
    with pytest.raises(ValueError, match="encode_only"):
        ren.query_gradient(pts, lat, encode_only=True)


def test_mesh_export_with_vertex_normals(sdfr, tmp_path):
    v = [[0.0, 0.5, -1.0], [1.0, 0.25, 0.125], [-0.5, 2.0, 3.0]]
    m = sdfr.Mesh(v, [[0, 1, 2]])
    assert m.vertex_normals is None
    m.vertex_normals = np.array([[0, 0, 1], [0.6, -0.8, 0], [-1, 0, 0]], np.float32)
    normals = ("v 0.00000000 0.50000000 -1.00000000\n"
               "v 1.00000000 0.25000000 0.12500000\n"
               "v -0.50000000 2.00000000 3.00000000\n"
               "vn 0.000000 0.000000 1.000000\n"
               "vn 0.600000 -0.800000 0.000000\n"
               "vn -1.000000 0.000000 0.000000\n"
               "f 1//1 2//2 3//3\n")
    path = tmp_path / "n.obj"
    assert m.export(str(path)) == normals
    assert path.read_text() == normals
    m.vertex_colors = np.array([[0, 0.5, 1], [0.25, 0.125, 0.75], [1, 1, 0]], np.float32)
    both = ("v 0.00000000 0.50000000 -1.00000000 0.000000 0.500000 1.000000\n"
            "v 1.00000000 0.25000000 0.12500000 0.250000 0.125000 0.750000\n"
            "v -0.50000000 2.00000000 3.00000000 1.000000 1.000000 0.000000\n"
            "vn 0.000000 0.000000 1.000000\n"
            "vn 0.600000 -0.800000 0.000000\n"
            "vn -1.000000 0.000000 0.000000\n"
            "f 1//1 2//2 3//3\n")
    assert m.export() == both
    m2 = sdfr.Mesh(v, [[0, 1, 2]], vertex_normals=m.vertex_normals)
    assert m2.export() == normals
    m2.vertex_normals = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="vertex_normals"):
        m2.export()


class _LinearField:
    """Renderer stub: sdf = a . p in network coordinates, so grad = a everywhere."""

    def __init__(self, a):
        self.a = torch.tensor(a, dtype=torch.float32)
        self.calls = []

    def query_gradient(self, points, styles, normalize=False, chunk_points=None):
        self.calls.append((tuple(points.shape), normalize))
        g = self.a.expand_as(points).clone()
        if normalize:
            g = g / g.norm(dim=-1, keepdim=True)
        return points @ self.a, g


def test_eikonal_residual_and_normal_mesh_on_a_known_field(sdfr):
    near, far = 0.88, 1.12
    # a unit world gradient is (far - near) / 2 in network coordinates
    unit = (far - near) / 2
    pts = torch.rand(2, 7, 3)
    lat = torch.zeros(2, 256)
    stub = _LinearField([0.0, unit, 0.0])
    res = sdfr.eikonal_residual(stub, lat, pts)
    assert res.shape == (2, 7)
    torch.testing.assert_close(res, torch.zeros(2, 7), rtol=0, atol=1e-6)
    res = sdfr.eikonal_residual(_LinearField([0.0, 3 * unit, 4 * unit]), lat, pts)
    torch.testing.assert_close(res, torch.full((2, 7), 4.0), rtol=0, atol=1e-5)
    res = sdfr.eikonal_residual(_LinearField([0.5, 0.0, 0.0]), lat, pts, near=0.0, far=2.0)
    torch.testing.assert_close(res, torch.full((2, 7), -0.5), rtol=0, atol=1e-6)
    # normal_mesh: the normalised gradient at world_to_network(vertices)
    m = sdfr.Mesh([[0.0, 0.01, 0.0], [0.02, 0.0, 0.0], [0.0, 0.0, 0.03]], [[0, 1, 2]])
    stub = _LinearField([0.0, 3.0, -4.0])
    n = sdfr.normal_mesh(m, stub, lat[:1])
    assert stub.calls == [((1, 3, 3), True)]
    assert n.dtype == np.float32 and n is m.vertex_normals
    np.testing.assert_allclose(n, np.tile(np.float32([0.0, 0.6, -0.8]), (3, 1)), atol=1e-7)
    assert m.export().count("\nvn ") == 3
    with pytest.raises(ValueError, match="one face"):
        sdfr.normal_mesh(m, stub, lat)

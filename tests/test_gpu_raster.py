"""GPU: the HIP mesh rasteriser against its fp32 / int64 definition (tests/raster_ref.py),
bit for bit, and what is built on it: attribute interpolation, render_mesh, noise
projection in NoiseInjection and through the Decoder."""
import numpy as np
import pytest
import torch

from tests import raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_raster_equals_ref(got, ref, what):
    fi, dep, bar = ref
    assert np.array_equal(got.face_idx.cpu().numpy(), fi), f"{what}: face_idx"
    assert np.array_equal(_bits(got.depth), _bits(dep)), f"{what}: depth bits"
    assert np.array_equal(_bits(got.bary), _bits(bar)), f"{what}: bary bits"


@pytest.fixture(scope="module")
def sphere():
    return R.icosphere(2, 0.1)


@pytest.fixture(scope="module")
def cams():
    """The three look-at cameras of the CPU comparison, as one batch."""
    return np.stack([R.look_at(az, el) for az, el, _ in R.VIEWS])


@pytest.fixture(scope="module")
def sphere_case(sdfr, sphere, cams):
    """7(a) at 32^2: the mesh, the batch of cameras, the HIP result and the reference (shared
    by the tests that only read them)."""
    v, f = sphere
    mesh = sdfr.Mesh(v, f)
    foc = [R.fov_focal(32)] * 3
    cam_t = torch.from_numpy(cams).to(DEV)
    foc_t = torch.tensor(foc, dtype=torch.float32, device=DEV)
    got = sdfr.rasterize_mesh(mesh, cam_t, foc_t, 32)
    ref = R.raster_ref(v, f, cams, foc, 32, 32)
    return dict(mesh=mesh, cam=cam_t, focal=foc_t, got=got, ref=ref)


def test_icosphere_batch_is_bit_equal(sdfr, sphere, cams, sphere_case):
    c = sphere_case
    assert c["got"].face_idx.shape == (3, 32, 32) and c["got"].face_idx.dtype == torch.int32
    assert c["got"].bary.shape == (3, 32, 32, 3)
    assert [int((c["ref"][0][b] >= 0).sum()) for b in range(2)] == [725, 728]
    _assert_raster_equals_ref(c["got"], c["ref"], "icosphere 32^2")
    # a non-square image, focal as [B,1,1]
    v, f = sphere
    foc = [R.fov_focal(32)] * 3
    got = sdfr.rasterize_mesh(c["mesh"], c["cam"], c["focal"].view(3, 1, 1), (48, 32))
    assert got.face_idx.shape == (3, 48, 32)
    _assert_raster_equals_ref(got, R.raster_ref(v, f, cams, foc, 48, 32), "icosphere 48x32")


def test_two_runs_are_bit_equal(sdfr, sphere_case):
    c = sphere_case
    again = sdfr.rasterize_mesh(c["mesh"], c["cam"], c["focal"], 32)
    for a, b in zip(again, c["got"]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)


IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)[None]


def _run_identity(sdfr, v, f, focal, res):
    mesh = sdfr.Mesh(v, f)
    got = sdfr.rasterize_mesh(mesh, torch.from_numpy(IDENTITY).to(DEV), float(focal), res)
    H, W = (res, res) if isinstance(res, int) else res
    return mesh, got, R.raster_ref(mesh.vertices, mesh.faces, IDENTITY, [focal], H, W)


def test_interpenetrating_triangles_depth_test_is_per_pixel(sdfr):
    """Two triangles that each cover most of a 64^2 image and cross each other: both boxes
    go through the large-box kernel, and each wins where it is nearer."""
    v = np.array([[-0.45, -0.45, -1.0], [0.45, -0.45, -1.6], [0.0, 0.45, -1.3],
                  [-0.45, -0.40, -1.6], [0.45, -0.40, -1.0], [0.0, 0.45, -1.3]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    _, got, ref = _run_identity(sdfr, v, f, 64.0, 64)
    ids = ref[0][0]
    assert (ids == 0).sum() > 300 and (ids == 1).sum() > 300
    _assert_raster_equals_ref(got, ref, "interpenetrating")


def test_shared_diagonal_through_pixel_centres(sdfr):
    """A quad split along a diagonal that passes exactly through pixel centres, and a second
    coplanar copy: edges are inclusive, nothing on the diagonal is lost, and the smallest id
    wins every exact tie."""
    res, focal = 16, 16.0                      # screen = 8 + 16 x, 8 - 16 y at z = -1: exact
    lo, hi = (2.5 - 8) / 16, (12.5 - 8) / 16
    quad = np.array([[lo, -lo, -1], [hi, -lo, -1], [hi, -hi, -1], [lo, -hi, -1]], np.float32)
    v = np.concatenate([quad, quad])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    _, got, ref = _run_identity(sdfr, v, f, focal, res)
    ids = got.face_idx[0].cpu().numpy()
    assert (ids >= 0).sum() == 11 * 11                       # pixels 2..12, edges included
    assert (np.diag(ids)[2:13] == 0).all()
    assert set(np.unique(ids)) == {-1, 0, 1}
    _assert_raster_equals_ref(got, ref, "diagonal")
    assert (_bits(got.depth[0])[ids >= 0] == _bits(np.float32(1.0))).all()


def test_culling_and_box_clamp(sdfr):
    v = np.array([
        [-0.2, -0.2, -1.0], [0.2, -0.2, -1.0], [0.0, 0.2, -0.005],    # 0: a vertex inside znear
        [-0.2, 0.0, -1.0], [0.0, 0.0, -1.0], [0.2, 0.0, -1.0],        # 1: zero area (collinear)
        [2.0, 2.0, -1.0], [2.5, 2.0, -1.0], [2.0, 2.5, -1.0],         # 2: wholly off screen
        [0.3, -0.1, -1.0], [0.9, -0.1, -1.0], [0.3, 0.3, -1.0],       # 3: half off screen
    ], np.float32)
    f = np.arange(12).reshape(4, 3)
    _, got, ref = _run_identity(sdfr, v, f, 32.0, 32)
    ids = got.face_idx[0].cpu().numpy()
    assert set(np.unique(ids)) == {-1, 3}
    assert (ids[:, -1] == 3).any()                           # it reaches the right border
    _assert_raster_equals_ref(got, ref, "culling")
    # a vertex behind the camera culls as well
    v[2] = [0.0, 0.2, 0.5]
    _, got, ref = _run_identity(sdfr, v, f, 32.0, 32)
    _assert_raster_equals_ref(got, ref, "culling, behind")


def test_boxes_on_both_sides_of_the_thread_walk_limit(sdfr, sphere, cams):
    """At 64^2 the icosphere's triangles have bounding boxes around 64 pixels, so some are
    walked by one thread and some by a wave; the reference has no such split."""
    v, f = sphere
    foc = R.fov_focal(64)
    X, Y, _, _, ok = R.project_ref(v, cams[0], foc, 32, 32, 0.01)
    assert ok.all()
    px = lambda q: ((q[f].max(1) - 2048) >> 12) - ((q[f].min(1) - 2048 + 4095) >> 12) + 1
    box = px(X) * px(Y)
    assert (box > 64).sum() > 20 and ((box <= 64) & (box > 0)).sum() > 20
    got = sdfr.rasterize_mesh(sdfr.Mesh(v, f), torch.from_numpy(cams[:1]).to(DEV), foc, 64)
    _assert_raster_equals_ref(got, R.raster_ref(v, f, cams[:1], [foc], 64, 64), "icosphere 64^2")


def test_more_large_boxes_than_waves(sdfr, sphere, cams):
    """At 128^2 every front triangle's box exceeds the thread-walk limit, and four views
    put more of them on the list (4 x 320, back faces included) than the large-box kernel
    has waves (1024): its waves take more than one entry each."""
    v, f = sphere
    four = np.concatenate([cams, R.look_at(0.7, -0.2)[None]])
    foc = [R.fov_focal(128)] * 4
    got = sdfr.rasterize_mesh(sdfr.Mesh(v, f), torch.from_numpy(four).to(DEV),
                              torch.tensor(foc, device=DEV), 128)
    X, Y, _, _, _ = R.project_ref(v, four[0], foc[0], 64, 64, 0.01)
    px = lambda q: ((q[f].max(1) - 2048) >> 12) - ((q[f].min(1) - 2048 + 4095) >> 12) + 1
    assert (px(X) * px(Y) > 64).sum() > 256
    _assert_raster_equals_ref(got, R.raster_ref(v, f, four, foc, 128, 128), "icosphere 4 x 128^2")


@pytest.mark.parametrize("C", (1, 3))
def test_interpolate_vertex_attributes(sdfr, sphere, sphere_case, C):
    c = sphere_case
    v, f = sphere
    fi, _, bar = c["ref"]
    rng = np.random.default_rng(C)
    attr = rng.standard_normal((len(v), C)).astype(np.float32)
    cov = torch.from_numpy(fi >= 0).to(DEV)[:, None].expand(3, C, 32, 32)
    out = sdfr.interpolate_vertex_attributes(c["mesh"], c["got"], attr, fill=-2.5)
    assert out.shape == (3, C, 32, 32)
    assert np.array_equal(_bits(out), _bits(R.interp_ref(attr, f, fi, bar, fill=-2.5)))
    assert (out[~cov] == -2.5).all()
    for nb in (1, 3):
        bg = rng.standard_normal((nb, C, 32, 32)).astype(np.float32)
        bg_t = torch.from_numpy(bg).to(DEV)
        out = sdfr.interpolate_vertex_attributes(c["mesh"], c["got"], torch.from_numpy(attr),
                                                 background=bg_t)
        assert np.array_equal(_bits(out), _bits(R.interp_ref(attr, f, fi, bar, background=bg)))
        assert torch.equal(out[~cov], bg_t.expand(3, C, 32, 32)[~cov])
    if C == 1:                                               # [V] is [V, 1]
        flat = sdfr.interpolate_vertex_attributes(c["mesh"], c["got"], attr[:, 0], fill=-2.5)
        assert np.array_equal(_bits(flat), _bits(R.interp_ref(attr, f, fi, bar, fill=-2.5)))
    with pytest.raises(ValueError):
        sdfr.interpolate_vertex_attributes(c["mesh"], c["got"], attr[:-1])


def test_render_mesh(sdfr, sphere, sphere_case):
    c = sphere_case
    v, f = sphere
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    colors = (0.5 + 4 * v).astype(np.float32)
    mesh = sdfr.Mesh(v, f, vertex_colors=colors, vertex_normals=normals)
    s = sdfr.render_mesh(mesh, c["cam"], c["focal"], 32)
    r = c["got"]
    hit = r.face_idx >= 0
    assert torch.equal(s.hit, hit[:, None].float())
    assert torch.equal(s.depth, r.depth[:, None])
    assert s.sample is None and s.residual is None and s.sdf is None
    assert torch.equal(s.xyz, sdfr.interpolate_vertex_attributes(mesh, r, v))
    n = sdfr.interpolate_vertex_attributes(mesh, r, normals)
    assert torch.equal(s.normal, n / n.norm(dim=1, keepdim=True).clamp_min(1e-20))
    assert torch.equal(s.rgb, sdfr.interpolate_vertex_attributes(mesh, r, colors))
    cov = hit[:, None].expand_as(s.normal)
    assert float((s.normal.norm(dim=1)[hit] - 1).abs().max()) < 1e-6
    assert (s.normal[~cov] == 0).all() and (s.xyz[~cov] == 0).all()
    # on a sphere about the origin the normal is the direction of the point itself
    assert float((s.normal - s.xyz / 0.1)[cov].abs().max()) < 0.05
    lit = sdfr.shade_surface(s)
    assert lit.shape == (3, 3, 32, 32) and torch.isfinite(lit).all()
    assert (lit[~cov] == 0).all() and float(lit.max()) > 0.3
    # without vertex normals: the triangle's own normal
    plain = sdfr.render_mesh(sdfr.Mesh(v, f), c["cam"], c["focal"], 32, want=("hit", "normal"))
    assert plain.rgb is None and plain.xyz is None and plain.depth is None
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    want = np.where((c["ref"][0] >= 0)[..., None], fn[np.maximum(c["ref"][0], 0)], 0)
    got = plain.normal.permute(0, 2, 3, 1).cpu().numpy()
    assert np.abs(got - want).max() < 1e-5
    with pytest.raises(ValueError):
        sdfr.render_mesh(mesh, c["cam"], c["focal"], 32, want=("sdf",))


def test_view_consistency(sdfr, sphere, sphere_case):
    """An attribute that is linear in position comes out as that function of the surface
    point in every view: of the interpolated position, and of the float64 point on the
    pixel's own ray."""
    c = sphere_case
    v, f = sphere
    coef, off = np.array([0.5, -0.3, 0.2], np.float32), np.float32(0.05)     # |coef|_1 = 1
    attr = (v @ coef + off).astype(np.float32)
    a = sdfr.interpolate_vertex_attributes(c["mesh"], c["got"], attr)[:, 0].cpu().numpy()
    xyz = sdfr.interpolate_vertex_attributes(c["mesh"], c["got"], v).cpu().numpy()
    fi, dep, _ = c["ref"]
    for b in range(2):
        cov = fi[b] >= 0
        lin = np.moveaxis(xyz[b], 0, -1).astype(np.float64) @ coef.astype(np.float64) + off
        assert np.abs(a[b] - lin)[cov].max() <= R.RAY_BOUND
        o, d = R.rays_ref(c["cam"][b].cpu().numpy(), float(c["focal"][b]), 32, 32)
        p = o + d * dep[b].astype(np.float64)[..., None]
        assert np.abs(a[b] - (p @ coef.astype(np.float64) + off))[cov].max() <= R.RAY_BOUND


def _seed_draw(seed, V):
    torch.manual_seed(seed)
    return torch.empty(V, 1).normal_()


def test_noise_injection_projects_through_the_mesh(sdfr, sphere, cams):
    v, f = sphere
    mesh = sdfr.Mesh(v, f)
    ni = sdfr.NoiseInjection(project=True).to(DEV)
    with torch.no_grad():
        ni.weight.fill_(0.1)
    r, foc = 64, R.fov_focal(64)
    cam = torch.from_numpy(cams[:1]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    image = torch.randn(1, 4, r, r, device=DEV, generator=g)
    noise = torch.randn(1, 1, r, r, device=DEV, generator=g)
    noise2 = torch.randn(1, 1, r, r, device=DEV, generator=g)

    def composed(vert_noise, camera, focal, background):
        raster = sdfr.rasterize_mesh(mesh, camera, focal, r)
        cov = (raster.face_idx >= 0)[:, None]
        assert 1000 < int(cov.sum()) < r * r
        interp = sdfr.interpolate_vertex_attributes(mesh, raster, vert_noise)
        return image + ni.weight * torch.where(cov, interp, background)

    with torch.no_grad():
        torch.manual_seed(11)
        out = ni(image, noise=noise, transform=cam, mesh_path=mesh, focal=foc)
        assert torch.equal(ni.vert_noise, _seed_draw(11, len(v)))
        assert torch.equal(out, composed(ni.vert_noise, cam, foc, noise))
        assert not torch.equal(out, image + ni.weight * noise)
        # another camera, another noise map: the first map stays the background, the
        # per-vertex noise stays what it was
        cam2 = torch.from_numpy(cams[1:2]).to(DEV)
        out2 = ni(image, noise=noise2, transform=cam2, mesh_path=mesh, focal=foc)
        assert torch.equal(ni.vert_noise, _seed_draw(11, len(v)))
        assert torch.equal(out2, composed(ni.vert_noise, cam2, foc, noise))
        # focal=None is the 12 degree field of view
        assert torch.equal(ni(image, noise=noise2, transform=cam, mesh_path=mesh), out)
        # noise=None: fresh noise, nothing projected
        torch.cuda.manual_seed(5)
        fresh = ni(image, noise=None, transform=cam, mesh_path=mesh, focal=foc)
        torch.cuda.manual_seed(5)
        assert torch.equal(fresh, image + ni.weight * image.new_empty(1, 1, r, r).normal_())
        # a mesh with another vertex count: the per-vertex noise is drawn again
        v1, f1 = R.icosphere(1, 0.1)
        torch.manual_seed(12)
        ni(image, noise=noise2, transform=cam, mesh_path=sdfr.Mesh(v1, f1), focal=foc)
        assert torch.equal(ni.vert_noise, _seed_draw(12, len(v1)))
        # B = 2 views of the one mesh, one shared background map
        ni.reset_projected_noise()
        assert ni.prev_noise is None and ni.vert_noise is None
        both = torch.from_numpy(cams[:2]).to(DEV)
        torch.manual_seed(11)
        out_b = ni(image.expand(2, -1, -1, -1), noise=noise, transform=both, mesh_path=mesh,
                   focal=foc)
        assert torch.equal(out_b[:1], out) and torch.equal(
            out_b[1:], composed(ni.vert_noise, cam2, foc, noise))
        with pytest.raises(ValueError):
            ni(image, noise=noise, transform=cam, mesh_path=None)


def _decoder(sdfr, seed=0):
    opt = sdfr.vol_render_opt()
    opt.model.project_noise = True
    opt.model.feature_encoder_in_channels = opt.rendering.width   # as Generator.__init__ sets it
    torch.manual_seed(seed)
    dec = sdfr.Decoder(opt.model).to(DEV).eval()
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, sdfr.NoiseInjection):
                m.weight.fill_(0.1)
            if isinstance(m, sdfr.FusedLeakyReLU):
                m.bias.normal_(0, 0.1)
    return dec


def _close(name, got, ref, atol, mean_tol):
    err = (got.double() - ref.double()).abs()
    print(f"{name}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
    assert float(err.max()) <= atol, f"{name}: max err {float(err.max()):.3e} > {atol:.1e}"
    assert float(err.mean()) <= mean_tol, f"{name}: mean err {float(err.mean()):.3e}"


def test_decoder_projected_noise_end_to_end(sdfr, sphere, cams, tmp_path, monkeypatch):
    v, f = sphere
    path = str(tmp_path / "identity.obj")
    sdfr.Mesh(v, f).export(path)
    dec = _decoder(sdfr)
    import sdface_gan_amd.raster as raster_mod
    calls = {"raster": 0, "interp": 0, "fused": 0}
    real_raster, real_interp = raster_mod.rasterize_mesh, raster_mod.interpolate_vertex_attributes
    real_fused = dec._fused_forward

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(raster_mod, "rasterize_mesh", count("raster", real_raster))
    monkeypatch.setattr(raster_mod, "interpolate_vertex_attributes", count("interp", real_interp))
    dec._fused_forward = count("fused", real_fused)
    feats = torch.randn(2, 256, 64, 64, device=DEV)
    z = torch.randn(2, 256, device=DEV)
    cam = torch.from_numpy(cams[:2]).to(DEV)
    focal = torch.full((2, 1, 1), R.fov_focal(64), device=DEV)
    kw = dict(randomize_noise=False, mesh_path=path)
    with torch.no_grad():
        fused, _ = dec(feats[:1], [z[:1]], transform=cam[:1], focal=focal[:1], **kw)
        assert calls == {"raster": 3, "interp": 5, "fused": 1}     # 64, 128, 256; five layers
        dec.use_fused = False
        mod, _ = dec(feats[:1], [z[:1]], transform=cam[:1], focal=focal[:1], **kw)
        dec.use_fused = True
        assert calls == {"raster": 6, "interp": 10, "fused": 1}
        plain, _ = dec(feats[:1], [z[:1]], transform=None, **kw)
        two, _ = dec(feats, [z], transform=cam, focal=focal, **kw)
        moved, _ = dec(feats[:1], [z[:1]], transform=cam[1:], focal=focal[:1], **kw)
    assert fused.shape == mod.shape == (1, 3, 256, 256) and two.shape == (2, 3, 256, 256)
    scale = float(mod.abs().max())
    atol, mtol = 1e-4 * max(1.0, scale), 1e-5 * max(1.0, scale)
    _close("projected fused vs module", fused, mod, atol, mtol)
    assert float((fused - plain).abs().max()) > 10 * atol
    _close("B = 2, first face", two[:1], fused, atol, mtol)
    # the noise follows the camera (same features, another pose)
    assert float((moved - fused).abs().max()) > 10 * atol
    # the mesh was read once, and reset forgets everything
    assert len(dec._proj.meshes) == 1 and dec.conv1.noise.prev_noise is not None
    dec.reset_projected_noise()
    assert not dec._proj.meshes and dec.conv1.noise.prev_noise is None
    assert all(sc.noise.vert_noise is None for sc in dec.convs)
    with pytest.raises(ValueError):
        dec(feats[:1], [z[:1]], transform=cam[:1], randomize_noise=False)


def test_generator_projected_call_stays_out_of_the_graph_cache(sdfr, sphere, tmp_path):
    from sdface_gan_amd.graphs import forward_cache
    v, f = sphere
    path = str(tmp_path / "identity.obj")
    sdfr.Mesh(v, f).export(path)
    opt = sdfr.vol_render_opt()
    opt.model.project_noise = True
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering).to(DEV).eval()
    with torch.no_grad():
        for m in g.decoder.modules():
            if isinstance(m, sdfr.NoiseInjection):
                m.weight.fill_(0.1)
    z = torch.randn(1, 256, device=DEV)
    cam, focal, near, far, _ = sdfr.generate_camera_params(64, DEV, batch=1)
    fused_calls = []
    real = g.decoder._fused_forward
    g.decoder._fused_forward = lambda *a, **k: (fused_calls.append(1), real(*a, **k))[1]
    outs = []
    with torch.no_grad():
        for _ in range(3):                                   # a sweep would be captured by now
            torch.manual_seed(9)
            outs.append(g([z], cam, focal, near, far, randomize_noise=False,
                          project_noise=True, mesh_path=path)[0])
        torch.manual_seed(9)
        plain = g([z], cam, focal, near, far, randomize_noise=False)[0]
    assert outs[0].shape == (1, 3, 256, 256) and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert not torch.equal(outs[0], plain)
    assert len(fused_calls) == 4                             # the HIP decoder every time
    cache = forward_cache(g)
    assert len(cache.graphs) == 0

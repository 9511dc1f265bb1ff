"""GPU parity: the fused HIP renderer (sdfr_render_ngp_forward) and the drop-in
Generator against the reference goldens and the oracle.

Bit-exact: the hash-grid features of every sample (encode stage), i.e. the
whole ray/sample/index chain.  Tolerances (fp32 MFMA vs. MKL summation order,
amplified by the SIREN gamma ~30) are stated per output below; they were set
from the measured error distribution with >= 4x margin.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (max, mean) |HIP - reference| bounds: ~3x the largest error measured on MI355X over
# every case that uses the key, f16x3 and fp32 fields alike (round 5,
# profiles/round5_parity.json; the per-case table is DESIGN.md §3).  The inputs are
# seeded and the kernels deterministic, so the errors are the same on every box: the
# bounds are regression tripwires for the split arithmetic, not noise allowances.
# Measured maxima (max / mean): features 2.9e-5 / 3.1e-6 (fp32 field, 8x8 one-sample
# case; f16x3 1.6e-5 / 1.8e-6), rgb 5.4e-7 / 1.3e-7, sdf 9.4e-7 / 1.7e-7, xyz 7.8e-8 /
# 9.1e-9, mask 4.2e-7 / 1.1e-7, 256^2 image 1.4e-5 / 2.2e-6; the op-by-op module path
# 1.1e-5 / 1.2e-6 (features), 4.2e-7 / 8.1e-8 (rgb); its golden faces 7.5e-6 / 7.9e-7,
# 3.6e-7 / 7.6e-8.  (Round 1-4 bounds: features 1.2e-4 / 1.5e-5, 4-10x looser.)
TOL = {"rgb": (1.2e-6, 3e-7), "features": (5e-5, 5e-6), "sdf": (2.5e-6, 4.5e-7),
       "xyz": (2.4e-7, 3e-8), "mask": (1.3e-6, 3.3e-7), "image": (4e-5, 7e-6),
       # the op-by-op PyTorch-ROCm path (training / eikonal) with the HIP encoders and
       # the reference's left-to-right rays_d (bit-exact, test_get_rays_on_device_bit_exact)
       "module_rgb": (1.3e-6, 2.5e-7), "module_features": (3.2e-5, 3.5e-6),
       "module_golden_rgb": (1.2e-6, 2.5e-7), "module_golden_features": (2.4e-5, 2.5e-6)}

_record = {}


def _cmp(name, key, got, ref, tol_key=None):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    err = np.abs(got - ref)
    _record[f"{name}:{key}"] = [float(err.max()), float(err.mean())]
    tmax, tmean = TOL[tol_key or key]
    assert err.max() <= tmax, f"{name}:{key} max err {err.max():.3e} > {tmax:.1e}"
    assert err.mean() <= tmean, f"{name}:{key} mean err {err.mean():.3e} > {tmean:.1e}"


def teardown_module(module):
    out = os.environ.get("SDFR_PARITY_JSON")
    if out:
        prev = {}
        if os.path.exists(out):
            with open(out) as f:
                prev = json.load(f)
        prev.update(_record)
        with open(out, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def renderer_sd(golden_dir):
    return W.det_state_dict(W.golden_entries(golden_dir), "renderer.")


_SD_CACHE = {}


def sd_for(golden_dir, amp):
    """Renderer state dict with the hash table at amplitude `amp` (tests/golden/weights.py)."""
    if amp not in _SD_CACHE:
        _SD_CACHE[amp] = W.det_state_dict(W.golden_entries(golden_dir), "renderer.",
                                          table_amp=amp)
    return _SD_CACHE[amp]


PRECISIONS = ["f16x3", "fp32"]


def make_renderer(sdfr, sd, res, N, precision="f16x3", **flags):
    opt = sdfr.vol_render_opt()
    r = opt.rendering
    r.N_samples = N
    for k, v in flags.items():
        r[k] = v
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res)
    own = ren.state_dict()
    ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()
                         if k[len("renderer."):] in own}, strict=True)
    ren.field_precision = precision
    return ren.to(DEV).eval()


def _inputs(g):
    t = lambda k: torch.from_numpy(g[k]).to(DEV)  # noqa: E731
    tr = torch.from_numpy(g["t_rand"]) if g["t_rand"].size else None
    return t("ext"), t("focal"), t("near"), t("far"), t("latent"), tr


CASES = [
    ("render_small", {}),
    ("render_mesh_opts", dict(static_viewdirs=True, force_background=True, perturb=0,
                              return_sdf=True, return_xyz=True)),
    ("render_face64", dict(return_sdf=True, return_xyz=True)),
    # hash table at the reference's init scale U(-1e-4, 1e-4) (grid.py:138-140) and a
    # trained-like U(-0.05, 0.05): the split-fp16 layer 0 scales each sample's
    # features by a power of two before the hi/lo split (field_p.h feat_scale)
    ("render_small_tab1e4", {}), ("render_small_tab05", {}),
    ("render_face64_tab1e4", {}), ("render_face64_tab05", {}),
]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name,flags", CASES)
def test_fused_render_vs_reference_golden(sdfr, golden_dir, name, flags, prec):
    g = np.load(golden_dir / f"{name}.npz")
    amp = float(g["table_amp"]) if "table_amp" in g.files else 1.0
    ren = make_renderer(sdfr, sd_for(golden_dir, amp), int(g["res"]), int(g["n_samples"]), prec,
                        **flags)
    cam, focal, near, far, lat, tr = _inputs(g)
    with torch.no_grad():
        assert ren._fused_ok(cam, lat, False)
        rgb, feat, sdf, mask, xyz, eik = ren(cam, focal, near, far, styles=lat, t_rand=tr)
    torch.cuda.synchronize()
    assert eik is None
    name = f"{name}_{prec}"
    _cmp(name, "rgb", rgb.cpu().numpy(), g["rgb"])
    _cmp(name, "features", feat.cpu().numpy(), g["features"])
    if "sdf" in g.files:
        _cmp(name, "sdf", sdf.cpu().numpy(), g["sdf"])
        _cmp(name, "xyz", xyz.cpu().numpy(), g["xyz"])
        _cmp(name, "mask", mask.cpu().numpy(), g["mask"])


def _tile_order_to_samples(enc, B, H, W, N):
    """[L][S_tile][2] (tile order, 16 rays per sample) -> [B*H*W*N, 32]."""
    L = 16
    tiles = (H * W + 15) // 16
    e = enc.reshape(L, B, tiles, N, 16, 2).transpose(1, 2, 4, 3, 0, 5)   # B,tile,n,s,L,2
    e = e.reshape(B, tiles * 16, N, L * 2)[:, :H * W]
    return e.reshape(B * H * W * N, L * 2)


@pytest.mark.parametrize("name", ["render_small", "render_face64"])
def test_encode_stage_bit_exact(sdfr, oracle_mod, golden_dir, renderer_sd, name):
    """Every sample's 32 hash-grid features equal the oracle's, bit for bit: this
    pins ray generation, sampling, normalisation, the grid index math and the gather's
    paired corner loads."""
    g = np.load(golden_dir / f"{name}.npz")
    res, N = int(g["res"]), int(g["n_samples"])
    ren = make_renderer(sdfr, renderer_sd, res, N)
    cam, focal, near, far, lat, tr = _inputs(g)
    B = cam.shape[0]
    with torch.no_grad():
        ws = ren.fused_forward(cam, focal, near, far, lat, t_rand=tr, encode_only=True)
    torch.cuda.synchronize()
    tiles = (res * res + 15) // 16
    S = B * tiles * N * 16
    enc = ws[: S * 16 * 2 * 4].view(torch.float32).cpu().numpy()
    got = _tile_order_to_samples(enc, B, res, res, N)
    ray = oracle_mod.sample_rays(g["ext"], g["focal"], g["near"], g["far"], res, res, N,
                                 t_rand=g["t_rand"])
    offsets, pls = oracle_mod.grid_offsets()
    emb = W.det_table(int(offsets[-1]), 2, seed=7)
    ref, _ = oracle_mod.grid_encode_forward(ray["grid_in"].reshape(-1, 3), emb, offsets, pls, 16)
    ref = ref.transpose(1, 0, 2).reshape(-1, 32)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("B,res,N,flags", [
    (3, 10, 7, {}),                                        # ragged tiles (100 rays), odd N
    (2, 8, 24, dict(no_offset_sampling=True)),             # stratified: per-sample t_rand
    (1, 16, 32, dict(perturb=0, static_viewdirs=True, force_background=True,
                     return_sdf=True, return_xyz=True)),
    (2, 8, 24, dict(no_z_normalize=True, return_xyz=True)),
    (2, 8, 16, dict(no_sdf=True)),                         # density branch (softplus)
    (1, 8, 1, {}),                                         # single sample per ray
])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fused_render_vs_oracle(sdfr, oracle_mod, renderer_sd, B, res, N, flags, prec):
    ren = make_renderer(sdfr, renderer_sd, res, N, prec, **flags)
    torch.manual_seed(B * 100 + res + N)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.from_numpy(W.det_uniform((B, 256), -1.5, 1.5, 5 + N))
    tr = None
    if flags.get("perturb", 1) > 0:
        tr = torch.rand((B, res, res, N) if flags.get("no_offset_sampling") else (B, res, res))
    with torch.no_grad():
        rgb, feat, sdf, mask, xyz, _ = ren(ext.to(DEV), focal.to(DEV), near.to(DEV),
                                           far.to(DEV), styles=lat.to(DEV), t_rand=tr)
    torch.cuda.synchronize()
    o = oracle_mod.render_ngp(
        renderer_sd, ext.numpy(), focal.numpy(), near.numpy(), far.numpy(), lat.numpy(), N=N,
        res=res, t_rand=None if tr is None else tr.numpy(),
        offset_sampling=not flags.get("no_offset_sampling", False),
        static_viewdirs=flags.get("static_viewdirs", False),
        z_normalize=not flags.get("no_z_normalize", False),
        force_background=flags.get("force_background", False),
        with_sdf=not flags.get("no_sdf", False))
    name = f"oracle_B{B}_r{res}_N{N}_{'_'.join(flags) or 'default'}_{prec}"
    _cmp(name, "rgb", rgb.cpu().numpy(), o["rgb"].numpy())
    _cmp(name, "features", feat.cpu().numpy(), o["features"].numpy())
    if sdf is not None:
        _cmp(name, "sdf", sdf.cpu().numpy(), o["sdf"].numpy())
    if xyz is not None:
        _cmp(name, "xyz", xyz.cpu().numpy(), o["xyz"].numpy())
        _cmp(name, "mask", mask.cpu().numpy(), o["mask"].numpy())


@pytest.mark.parametrize("prec", PRECISIONS)
def test_out_of_bound_samples(sdfr, oracle_mod, renderer_sd, prec):
    """Camera far outside the unit volume: normalized points leave [0,1]^3 and the
    grid contributes exactly zero (gridencoder.cu:110-135)."""
    ren = make_renderer(sdfr, renderer_sd, 8, 24, prec)
    torch.manual_seed(3)
    ext, focal, near, far, _ = sdfr.generate_camera_params(8, "cpu", batch=1)
    ext[:, :, 3] *= 3.0
    lat = torch.from_numpy(W.det_uniform((1, 256), -1, 1, 3))
    tr = torch.rand(1, 8, 8)
    with torch.no_grad():
        rgb, feat, *_ = ren(ext.to(DEV), focal.to(DEV), near.to(DEV), far.to(DEV),
                            styles=lat.to(DEV), t_rand=tr)
    o = oracle_mod.render_ngp(renderer_sd, ext.numpy(), focal.numpy(), near.numpy(),
                              far.numpy(), lat.numpy(), N=24, res=8, t_rand=tr.numpy(),
                              return_intermediates=True)
    assert (o["enc"].abs().sum(-1) == 0).any()
    _cmp(f"oob_{prec}", "rgb", rgb.cpu().numpy(), o["rgb"].numpy())
    _cmp(f"oob_{prec}", "features", feat.cpu().numpy(), o["features"].numpy())


def test_fused_equals_unfused_module_path(sdfr, oracle_mod, renderer_sd):
    """The autograd path (HIP encoders + PyTorch-ROCm MLP/compositing ops) and the
    fused kernel both match the oracle; the module path carries torch-ROCm's own
    GEMM/transcendental rounding, hence its separate, looser bound."""
    ren = make_renderer(sdfr, renderer_sd, 16, 24)
    torch.manual_seed(8)
    ext, focal, near, far, _ = sdfr.generate_camera_params(16, "cpu", batch=2)
    lat = torch.from_numpy(W.det_uniform((2, 256), -1, 1, 8))
    tr = torch.rand(2, 16, 16)
    args = [t.to(DEV) for t in (ext, focal, near, far)]
    with torch.no_grad():
        f = ren(*args, styles=lat.to(DEV), t_rand=tr)
        ren.use_fused = False
        u = ren(*args, styles=lat.to(DEV), t_rand=tr)
    o = oracle_mod.render_ngp(renderer_sd, ext.numpy(), focal.numpy(), near.numpy(),
                              far.numpy(), lat.numpy(), N=24, res=16, t_rand=tr.numpy())
    _cmp("fused", "rgb", f[0].cpu().numpy(), o["rgb"].numpy())
    _cmp("fused", "features", f[1].cpu().numpy(), o["features"].numpy())
    _cmp("module", "rgb", u[0].cpu().numpy(), o["rgb"].numpy(), "module_rgb")
    _cmp("module", "features", u[1].cpu().numpy(), o["features"].numpy(), "module_features")


def test_generator_vs_reference_golden(sdfr, golden_dir):
    z = np.load(golden_dir / "generator.npz")
    opt = sdfr.vol_render_opt()
    g = sdfr.Generator(opt.model, opt.rendering)
    W.det_init_(g)
    g = g.to(DEV).eval()
    t = lambda k: torch.from_numpy(z[k]).to(DEV)  # noqa: E731
    with torch.no_grad():
        rgb, thumb = g([t("z")], t("ext"), t("focal"), t("near"), t("far"),
                       randomize_noise=False, t_rand=torch.from_numpy(z["t_rand"]))
    _cmp("generator", "thumb", thumb.cpu().numpy(), z["thumb"], "rgb")
    # the 256^2 image: the fused HIP decoder on top (split-fp16 implicit-GEMM convolutions
    # with the styled epilogues, csrc/conv_f16x3.hip, csrc/decoder.hip)
    _cmp("generator", "image", rgb.cpu().numpy(), z["rgb"])


@pytest.mark.parametrize("prec", PRECISIONS)
def test_batch_consistency(sdfr, renderer_sd, prec):
    """Faces are independent: rendering B faces at once == one at a time (bitwise)."""
    ren = make_renderer(sdfr, renderer_sd, 16, 24, prec)
    torch.manual_seed(4)
    ext, focal, near, far, _ = sdfr.generate_camera_params(16, DEV, batch=3)
    lat = torch.from_numpy(W.det_uniform((3, 256), -1, 1, 4)).to(DEV)
    tr = torch.rand(3, 16, 16)
    with torch.no_grad():
        full = ren(ext, focal, near, far, styles=lat, t_rand=tr)
        for b in range(3):
            one = ren(ext[b:b + 1], focal[b:b + 1], near[b:b + 1], far[b:b + 1],
                      styles=lat[b:b + 1], t_rand=tr[b:b + 1])
            assert torch.equal(one[0], full[0][b:b + 1])
            assert torch.equal(one[1], full[1][b:b + 1])


# ---------------------------------------------------------------- SIREN (type "sdf")
@pytest.fixture(scope="module")
def siren_sd(golden_dir):
    return W.det_state_dict(W.golden_entries(golden_dir, siren=True), "renderer.")


@pytest.mark.parametrize("net", ["ngp", "siren"])
@pytest.mark.parametrize("B", [1, 4])
def test_fused_render_deterministic(sdfr, renderer_sd, siren_sd, net, B):
    """Repeated renders of the same inputs are bit-identical: every cross-wave hand-off
    of the field kernel (weight ring, exchange slots, sigma / alpha / colour half-sums)
    is ordered by its barriers.  (A scalar branch inside the LDS-DMA asm once let MFMA
    results be read before they landed: colour-feature rows changed run to run.)"""
    if net == "ngp":
        ren = make_renderer(sdfr, renderer_sd, 64, 24, "f16x3", return_sdf=True, return_xyz=True)
    else:
        ren = make_siren(sdfr, siren_sd, 64, 24, return_sdf=True, return_xyz=True)
    torch.manual_seed(11)
    ext, focal, near, far, _ = sdfr.generate_camera_params(64, DEV, batch=B)
    lat = torch.from_numpy(W.det_uniform((B, 256), -1, 1, 5)).to(DEV)
    tr = torch.rand(B, 64, 64)
    with torch.no_grad():
        runs = [ren(ext, focal, near, far, styles=lat, t_rand=tr) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            if torch.is_tensor(a):
                assert torch.equal(a, b)


def make_siren(sdfr, sd, res, N, **flags):
    opt = sdfr.vol_render_opt(ngp=False)
    r = opt.rendering
    r.N_samples = N
    for k, v in flags.items():
        r[k] = v
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res)
    own = ren.state_dict()
    ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()
                         if k[len("renderer."):] in own}, strict=True)
    return ren.to(DEV).eval()


SIREN_CASES = [
    ("render_siren_small", {}),
    ("render_siren_mesh_opts", dict(static_viewdirs=True, force_background=True, perturb=0,
                                    return_sdf=True, return_xyz=True)),
    ("render_siren_face32", dict(return_sdf=True, return_xyz=True)),
]


@pytest.mark.parametrize("name,flags", SIREN_CASES)
def test_fused_siren_vs_reference_golden(sdfr, golden_dir, siren_sd, name, flags):
    """The fused SIREN kernel (sdfr_render_siren_forward) against the reference's
    own SirenGenerator renderer on the same inputs."""
    g = np.load(golden_dir / f"{name}.npz")
    ren = make_siren(sdfr, siren_sd, int(g["res"]), int(g["n_samples"]), **flags)
    cam, focal, near, far, lat, tr = _inputs(g)
    with torch.no_grad():
        assert ren._fused_ok(cam, lat, False)
        rgb, feat, sdf, mask, xyz, eik = ren(cam, focal, near, far, styles=lat, t_rand=tr)
    torch.cuda.synchronize()
    _cmp(name, "rgb", rgb.cpu().numpy(), g["rgb"])
    _cmp(name, "features", feat.cpu().numpy(), g["features"])
    if "sdf" in g.files:
        _cmp(name, "sdf", sdf.cpu().numpy(), g["sdf"])
        _cmp(name, "xyz", xyz.cpu().numpy(), g["xyz"])
        _cmp(name, "mask", mask.cpu().numpy(), g["mask"])


@pytest.mark.parametrize("B,res,N,flags", [
    (3, 10, 7, {}),                                        # ragged tiles, odd N
    (2, 8, 24, dict(no_offset_sampling=True)),
    (2, 8, 24, dict(no_z_normalize=True, return_xyz=True)),
    (2, 8, 16, dict(no_sdf=True)),
])
def test_fused_siren_vs_oracle(sdfr, oracle_mod, siren_sd, B, res, N, flags):
    ren = make_siren(sdfr, siren_sd, res, N, **flags)
    torch.manual_seed(B * 100 + res + N + 1)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, "cpu", batch=B)
    lat = torch.from_numpy(W.det_uniform((B, 256), -1.5, 1.5, 9 + N))
    tr = torch.rand((B, res, res, N) if flags.get("no_offset_sampling") else (B, res, res))
    with torch.no_grad():
        rgb, feat, sdf, mask, xyz, _ = ren(ext.to(DEV), focal.to(DEV), near.to(DEV),
                                           far.to(DEV), styles=lat.to(DEV), t_rand=tr)
    torch.cuda.synchronize()
    o = oracle_mod.render_siren(
        siren_sd, ext.numpy(), focal.numpy(), near.numpy(), far.numpy(), lat.numpy(), N=N,
        res=res, t_rand=tr.numpy(), offset_sampling=not flags.get("no_offset_sampling", False),
        z_normalize=not flags.get("no_z_normalize", False),
        with_sdf=not flags.get("no_sdf", False))
    name = f"siren_oracle_B{B}_r{res}_N{N}_{'_'.join(flags) or 'default'}"
    _cmp(name, "rgb", rgb.cpu().numpy(), o["rgb"].numpy())
    _cmp(name, "features", feat.cpu().numpy(), o["features"].numpy())
    if xyz is not None:
        _cmp(name, "xyz", xyz.cpu().numpy(), o["xyz"].numpy())
        _cmp(name, "mask", mask.cpu().numpy(), o["mask"].numpy())


def test_siren_fused_equals_module_path(sdfr, siren_sd):
    """Fused kernel vs. the op-by-op PyTorch-ROCm SirenGenerator on the same GPU
    inputs (module-path bound: torch-ROCm's own GEMM / sin rounding)."""
    ren = make_siren(sdfr, siren_sd, 16, 24)
    torch.manual_seed(12)
    ext, focal, near, far, _ = sdfr.generate_camera_params(16, DEV, batch=2)
    lat = torch.from_numpy(W.det_uniform((2, 256), -1, 1, 12)).to(DEV)
    tr = torch.rand(2, 16, 16)
    with torch.no_grad():
        f = ren(ext, focal, near, far, styles=lat, t_rand=tr)
        ren.use_fused = False
        u = ren(ext, focal, near, far, styles=lat, t_rand=tr)
    _cmp("siren_module", "rgb", f[0].cpu().numpy(), u[0].cpu().numpy(), "module_rgb")
    _cmp("siren_module", "features", f[1].cpu().numpy(), u[1].cpu().numpy(), "module_features")


def test_graphed_generator_matches_eager(sdfr):
    """HIP-graph replay of the whole inference forward (sdface-gan_amd/graphs.py):
    the same images as the eager forward, bit for bit, from the same device-RNG
    state (decoder noise and sampling offsets are drawn inside the graph), a fresh
    draw on every replay, and new latents/cameras picked up from the inputs."""
    dev = torch.device("cuda", 0)
    opt = sdfr.vol_render_opt()
    torch.manual_seed(3)
    g = sdfr.Generator(opt.model, opt.rendering).to(dev).eval()
    g.renderer.rng_device = "device"
    gg = sdfr.GraphedGenerator(g)
    for B in (1, 3):
        z = torch.randn(B, 256, device=dev)
        cam, focal, near, far, _ = sdfr.generate_camera_params(64, dev, batch=B)
        torch.cuda.manual_seed(11)
        with torch.no_grad():
            ref_rgb, ref_thumb = g([z], cam, focal, near, far)
        gg(z, cam, focal, near, far)                  # capture (+ warmup draws)
        torch.cuda.manual_seed(11)
        rgb, thumb = gg(z, cam, focal, near, far)
        torch.cuda.synchronize()
        assert rgb.shape == (B, 3, 256, 256) and thumb.shape == (B, 3, 64, 64)
        assert torch.equal(rgb, ref_rgb) and torch.equal(thumb, ref_thumb)
        first = rgb.clone()
        rgb2, _ = gg(z, cam, focal, near, far)        # next draw of noise / offsets
        assert not torch.equal(rgb2, first)
        z2 = torch.randn(B, 256, device=dev)
        torch.cuda.manual_seed(12)
        with torch.no_grad():
            ref2, _ = g([z2], cam, focal, near, far)
        torch.cuda.manual_seed(12)
        got2, _ = gg(z2, cam, focal, near, far)
        assert torch.equal(got2, ref2)


@pytest.mark.parametrize("rng_device", ["cpu", "device"])
def test_forward_graph_cache_matches_uncached(sdfr, rng_device):
    """Generator.forward's own graph cache (graphs.py ForwardGraphCache, eval.py's
    unchanged loop): a run of plain inference calls with new latents and cameras each
    -- eager on the first sighting, captured on the second, replayed after -- gives
    the uncached path's images bit for bit from the same RNG state (CPU stream for
    the reference's host-drawn sampling offsets, device stream for the decoder noise),
    leaves both streams where the uncached run leaves them, returns outputs a later
    call does not overwrite, and re-captures after a weight update."""
    dev = torch.device("cuda", 0)
    opt = sdfr.vol_render_opt()
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering).to(dev).eval()
    g.renderer.rng_device = rng_device
    from sdface_gan_amd.graphs import forward_cache

    def run(cached, n=4, B=1):
        g.graph_inference = cached
        torch.manual_seed(21)
        outs = []
        for _ in range(n):
            z = torch.randn(B, 256, device=dev)
            cam, focal, near, far, _ = sdfr.generate_camera_params(64, dev, batch=B)
            with torch.no_grad():
                outs.append(g([z], cam, focal, near, far, truncation=1,
                              truncation_latent=None))
        torch.cuda.synchronize()
        return outs, torch.get_rng_state(), torch.cuda.get_rng_state(dev)

    ref, cpu_ref, dev_ref = run(False)
    got, cpu_got, dev_got = run(True)
    assert len(forward_cache(g).graphs) == 1            # captured once, then replayed
    for (r_rgb, r_th), (g_rgb, g_th) in zip(ref, got):
        assert torch.equal(g_rgb, r_rgb) and torch.equal(g_th, r_th)
    assert not torch.equal(got[2][0], got[3][0])        # each replay its own output
    assert torch.equal(cpu_got, cpu_ref) and torch.equal(dev_got, dev_ref)
    # a weight update (EMA-style in-place step) drops the graph; results follow it
    with torch.no_grad():
        for p in g.decoder.parameters():
            p.mul_(0.999)
    ref2, _, _ = run(False, n=3)
    got2, _, _ = run(True, n=3)
    for (r_rgb, _), (g_rgb, _) in zip(ref2, got2):
        assert torch.equal(g_rgb, r_rgb)
    assert not torch.equal(ref2[0][0], ref[0][0])


@pytest.mark.parametrize("B,res,N", [(1, 64, 24), (2, 64, 24), (1, 32, 18), (3, 10, 7)])
def test_field_sample_split_matches_whole_rays(sdfr, renderer_sd, B, res, N):
    """Small batches split each ray's samples over up to 4 workgroups and chain the
    segments (renderer.max_field_segments, per call); the result equals the whole-ray march
    up to the re-associated transmittance product (fp32 rounding)."""
    ren = make_renderer(sdfr, renderer_sd, res, N, return_sdf=True, return_xyz=True)
    torch.manual_seed(B * 100 + res + N)
    cam, focal, near, far, _ = sdfr.generate_camera_params(res, DEV, batch=B)
    lat = torch.randn(B, 256, device=DEV)
    tr = torch.rand(B, res, res)
    outs = []
    for m in (1, 4):
        ren.max_field_segments = m
        with torch.no_grad():
            outs.append([t.clone() for t in ren(cam, focal, near, far, styles=lat,
                                                t_rand=tr)[:5]])
    (rgb1, f1, sdf1, m1, x1), (rgb4, f4, sdf4, m4, x4) = outs
    assert torch.equal(sdf1, sdf4)                      # per-sample heads: unchanged
    torch.testing.assert_close(rgb4, rgb1, rtol=0, atol=2e-6)
    torch.testing.assert_close(f4, f1, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(x4, x1, rtol=0, atol=2e-6)
    torch.testing.assert_close(m4, m1, rtol=1e-5, atol=1e-7)


def test_graphed_random_faces_matches_eager(sdfr):
    """GraphedGenerator.random_faces: latents and cameras drawn inside the graph,
    the same images as eval.py's eager loop body from the same RNG state."""
    dev = torch.device("cuda", 0)
    opt = sdfr.vol_render_opt()
    torch.manual_seed(4)
    g = sdfr.Generator(opt.model, opt.rendering).to(dev).eval()
    g.renderer.rng_device = "device"
    gg = sdfr.GraphedGenerator(g)
    gg.random_faces(2, 64)                               # capture
    torch.cuda.manual_seed(21)
    rgb, thumb = gg.random_faces(2, 64)
    torch.cuda.manual_seed(21)
    with torch.no_grad():
        z = torch.randn(2, 256, device=dev)
        cam, focal, near, far, _ = sdfr.generate_camera_params(64, dev, batch=2)
        ref_rgb, ref_thumb = g([z], cam, focal, near, far)
    assert torch.equal(rgb, ref_rgb) and torch.equal(thumb, ref_thumb)
    first = rgb.clone()
    assert not torch.equal(gg.random_faces(2, 64)[0], first)


# ---------------------------------------------------------------- camera / rays on the GPU
def test_camera_on_device_matches_reference(sdfr, golden_dir, monkeypatch):
    """generate_camera_params on cuda (its own op sequence: `up` built in place, the
    degenerate-axis replacement always formed, camera.py) against the reference's
    CPU results (sdf_utils.py:97-159): injected locations incl. straight-down / up
    rows, and the gauss / uniform / sweep branches with the reference's CPU draws
    injected.  Bound 1e-6 absolute (a few fp32 ulp of the unit-scale entries: torch-ROCm's
    sin / cos / normalize vs torch-CPU's); the measured error goes to the parity record."""
    from importlib import import_module
    cam_mod = import_module(sdfr.generate_camera_params.__module__)
    g = np.load(golden_dir / "camera.npz")

    def check(out, prefix):
        for k, v in zip(["ext", "focal", "near", "far", "vp"], out):
            ref = g[f"{prefix}_{k}"]
            err = np.abs(v.cpu().numpy().astype(np.float64) - ref)
            _record[f"camera_{prefix}:{k}"] = [float(err.max()), float(err.mean())]
            assert err.max() <= 1e-6, f"camera {prefix}_{k}: max err {err.max():.3e}"

    locs = torch.from_numpy(g["loc_locations"])
    check(sdfr.generate_camera_params(128, DEV, batch=locs.shape[0], locations=locs.to(DEV)),
          "loc")
    real_rand, real_randn = torch.rand, torch.randn

    def cpu_draw(fn):
        def draw(*shape, device=None, **kw):
            return fn(*shape, **kw).to(device)
        return draw
    monkeypatch.setattr(cam_mod.torch, "rand", cpu_draw(real_rand))
    monkeypatch.setattr(cam_mod.torch, "randn", cpu_draw(real_randn))
    # the gauss branch draws through _scaled_randn (normal_(0, s)): the reference's
    # scale * randn on the CPU stands in for it (test_scaled_randn_is_scale_times_randn)
    monkeypatch.setattr(cam_mod, "_scaled_randn",
                        lambda n, s, device: (s * real_randn(n, 1)).view(-1).to(device))
    for name, kw in [("gauss", {}), ("uniform", {"uniform": True}), ("sweep", {"sweep": True})]:
        torch.manual_seed(123)
        out = sdfr.generate_camera_params(64, DEV, batch=5, **kw)
        assert out[0].is_cuda
        check(out, name)


def test_scaled_randn_is_scale_times_randn(sdfr):
    """The GPU camera branch's one-launch draw normal_(0, s) equals the reference's
    s * torch.randn(n, 1) (sdf_utils.py:118-119) bit for bit from the same generator
    state, and leaves the generator where the reference's draw leaves it."""
    from importlib import import_module
    cam_mod = import_module(sdfr.generate_camera_params.__module__)
    for n, s in [(1, 0.3), (5, 0.15), (32, 0.3), (1000, 0.7)]:
        torch.manual_seed(11)
        ref = (s * torch.randn(n, 1, device=DEV)).view(-1)
        after_ref = torch.randn(3, device=DEV)
        torch.manual_seed(11)
        got = cam_mod._scaled_randn(n, s, DEV)
        after_got = torch.randn(3, device=DEV)
        assert torch.equal(got, ref), (n, s)
        assert torch.equal(after_got, after_ref), (n, s)


def test_get_rays_on_device_bit_exact(sdfr, golden_dir):
    """The module path's rays on cuda equal the reference's CPU rays bit for bit
    (explicit left-to-right sum), so its hash cells are the reference's."""
    g = np.load(golden_dir / "render_small.npz")
    opt = sdfr.vol_render_opt()
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256,
                                     out_im_res=int(g["res"])).to(DEV)
    _, rays_d, _ = ren.get_rays(torch.from_numpy(g["focal"]).to(DEV),
                                torch.from_numpy(g["ext"]).to(DEV))
    np.testing.assert_array_equal(rays_d.cpu().numpy(), g["rays_d"])


@pytest.mark.parametrize("name", ["render_small", "render_small_tab05"])
def test_module_path_vs_reference_golden(sdfr, golden_dir, name):
    """The op-by-op path (HIP encoders + PyTorch-ROCm GEMMs / sin) on the reference
    golden: with bit-exact rays its error is GEMM-order rounding amplified by the
    SIREN gain, like the fused kernel's (bound 'module_golden')."""
    g = np.load(golden_dir / f"{name}.npz")
    amp = float(g["table_amp"]) if "table_amp" in g.files else 1.0
    ren = make_renderer(sdfr, sd_for(golden_dir, amp), int(g["res"]), int(g["n_samples"]))
    ren.use_fused = False
    cam, focal, near, far, lat, tr = _inputs(g)
    with torch.no_grad():
        rgb, feat, *_ = ren(cam, focal, near, far, styles=lat, t_rand=tr)
    _cmp(f"module_{name}", "rgb", rgb.cpu().numpy(), g["rgb"], "module_golden_rgb")
    _cmp(f"module_{name}", "features", feat.cpu().numpy(), g["features"],
         "module_golden_features")


def test_graft_entry_smoke():
    """__graft_entry__.smoke() (the round-end smoke check): the fused render against
    the oracle and Generator.forward's thumbnail equal to the renderer's own output."""
    import __graft_entry__
    __graft_entry__.smoke()


@pytest.mark.parametrize("B,fc", [(8, False), (4, True)])
def test_feature_split_store_matches_modulate_pass(sdfr, B, fc):
    """Generator.forward with the field kernel writing the decoder's first input
    (features x modulation in split-NHWC, ABI 12) gives the images of the NCHW features
    + modulate_nhwc path bit for bit (same fp32 product, same round-to-nearest hi / lo
    split; the product pinned so hipcc cannot fold it into a one-rounding v_fma_mix)."""
    dev = torch.device("cuda", 0)
    opt = sdfr.vol_render_opt(ngp=not fc, fc=fc)
    torch.manual_seed(7)
    g = sdfr.Generator(opt.model, opt.rendering).to(dev).eval()
    g.renderer.rng_device = "device"
    z = torch.randn(B, 256, device=dev)
    cam, focal, near, far, _ = sdfr.generate_camera_params(64, dev, batch=B)
    outs = []
    for split in (False, True, True):
        g.fuse_feature_split = split
        torch.cuda.manual_seed(31)
        with torch.no_grad():
            outs.append(g([z], cam, focal, near, far))
    torch.cuda.synchronize()
    for rgb, thumb in outs[1:]:
        assert torch.equal(rgb, outs[0][0]) and torch.equal(thumb, outs[0][1])


@pytest.mark.parametrize("B", [1, 3])
def test_feature_split_store_through_segment_merge(sdfr, B):
    """The split-NHWC feature store of the segment-merge kernel (small batches, where
    the Generator keeps the NCHW path) equals sdfr_modulate_to_nhwc_split of the NCHW
    features of the same render, bit for bit."""
    from sdface_gan_amd import decoder_ops as ops
    dev = torch.device("cuda", 0)
    opt = sdfr.vol_render_opt()
    torch.manual_seed(9)
    g = sdfr.Generator(opt.model, opt.rendering).to(dev).eval()
    ren = g.renderer
    cam, focal, near, far, _ = sdfr.generate_camera_params(64, dev, batch=B)
    lat = torch.randn(B, 256, device=dev)
    mod = torch.rand(B, 256, device=dev) + 0.5
    tr = torch.rand(B, 64, 64, device=dev)
    with torch.no_grad():
        o1 = ren.fused_forward(cam, focal, near, far, lat, t_rand=tr)
        o2 = ren.fused_forward(cam, focal, near, far, lat, t_rand=tr, feat_mod=mod)
    assert torch.equal(o1[0], o2[0])
    assert torch.equal(o2[1], ops.modulate_to_nhwc_split(o1[1], mod))


def test_decoder_prep_overlap_matches_in_order(sdfr):
    """Generator.forward's decoder prep on the side stream (batch >= 8, warm weight
    caches) gives the images of the in-order prep from the same RNG state, and the
    generator still deep-copies after it ran (the stream is kept off the module)."""
    import copy
    dev = torch.device("cuda", 0)
    opt = sdfr.vol_render_opt()
    torch.manual_seed(5)
    g = sdfr.Generator(opt.model, opt.rendering).to(dev).eval()
    g.renderer.rng_device = "device"
    B = 8
    z = torch.randn(B, 256, device=dev)
    cam, focal, near, far, _ = sdfr.generate_camera_params(64, dev, batch=B)
    outs = []
    for overlap in (False, True, True):       # the 2nd call warms the caches
        g.overlap_decoder_prep = overlap
        torch.cuda.manual_seed(21)
        with torch.no_grad():
            outs.append(g([z], cam, focal, near, far))
    torch.cuda.synchronize()
    for rgb, thumb in outs[1:]:
        assert torch.equal(rgb, outs[0][0]) and torch.equal(thumb, outs[0][1])
    copy.deepcopy(g)

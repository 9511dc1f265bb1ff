"""CPU: the C-ABI library, the drop-in module surface and the PyTorch parts."""
import ast
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.golden import weights as W

REPO = Path(__file__).resolve().parents[1]


def header_symbols():
    """Functions include/sdfr.h declares."""
    txt = (REPO / "include" / "sdfr.h").read_text()
    return sorted(set(re.findall(r"^\s*(?:int|size_t|const char \*)\s*(sdfr_\w+)\s*\(", txt, re.M)))


def library_symbols(path):
    """Global text symbols with the sdfr_ prefix that a shared library exports."""
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                         text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines()
                   if ln.split()[-2:-1] == ["T"] and ln.split()[-1].startswith("sdfr_")})


def test_library_exports_every_header_symbol(sdfr):
    lib = sdfr._lib.lib()
    syms = header_symbols()
    assert len(syms) >= 9
    for s in syms:
        assert hasattr(lib, s), s
    assert set(syms) == set(sdfr._lib.EXPORTS)
    assert lib.sdfr_abi_version() == sdfr._lib.ABI_VERSION
    # the library exports exactly the documented entry points
    exported = library_symbols(sdfr._lib.LIB_PATH)
    assert exported == syms
    # There is one build.  The header declares nothing under a build macro (its only
    # conditionals are the include guard and the C++ linkage block; the profiling-build
    # block it had up to commit a4b3009 is gone), and no debug setter that selects a
    # kernel variant through process-global state is declared or exported.
    header = (REPO / "include" / "sdfr.h").read_text()
    conds = re.findall(r"^\s*#\s*(?:ifdef|ifndef|if|elif)\s+(.*)$", header, re.M)
    assert sorted(conds) == ["SDFR_H_", "__cplusplus", "__cplusplus"]
    for s in exported + syms:
        assert not s.startswith("sdfr_debug_set_"), s


def test_argument_errors_mirror_reference(sdfr):
    """Rejections happen before any launch, so they are checkable without a GPU."""
    lib = sdfr._lib.lib()
    nul = None
    rc = lib.sdfr_grid_encode_forward(nul, nul, nul, nul, 4, 3, 3, 16, 0.5, 16, nul, 0, 0, 0, nul)
    assert rc == sdfr._lib.SDFR_EINVAL
    assert b"C must be 1, 2, 4, or 8" in lib.sdfr_last_error()
    rc = lib.sdfr_grid_encode_forward(nul, nul, nul, nul, 4, 6, 2, 16, 0.5, 16, nul, 0, 0, 0, nul)
    assert rc == sdfr._lib.SDFR_EINVAL
    rc = lib.sdfr_sh_encode_forward(nul, nul, 4, 2, 4, nul, nul)
    assert rc == sdfr._lib.SDFR_EINVAL and b"input dim == 3" in lib.sdfr_last_error()
    rc = lib.sdfr_sh_encode_forward(nul, nul, 4, 3, 9, nul, nul)
    assert rc == sdfr._lib.SDFR_EINVAL
    rc = lib.sdfr_sh_encode_forward(nul, nul, 4, 3, 6, nul, nul)   # degrees 5..8 exist:
    assert rc == sdfr._lib.SDFR_EINVAL and b"null tensor" in lib.sdfr_last_error()
    w, a = sdfr._lib.NgpWeights(), sdfr._lib.NgpRenderArgs()
    rc = lib.sdfr_render_ngp_forward(ctypes.byref(w), ctypes.byref(a), nul)
    assert rc in (sdfr._lib.SDFR_EINVAL, sdfr._lib.SDFR_EUNSUPPORTED)
    with pytest.raises(RuntimeError, match="sdfr_render_ngp_forward"):
        sdfr._lib.check(rc, "sdfr_render_ngp_forward")


def test_workspace_size(sdfr):
    lib = sdfr._lib.lib()
    n = lib.sdfr_render_ngp_workspace_bytes(2, 64, 64, 24, 16)
    enc = 2 * 4096 * 24 * 16 * 2 * 4
    fixed = 67 * 1024 * 16 + 2 * 8 * 256 * 4          # fp32 fragments + FiLM vectors
    # split-fp16 fragments (51 slices of one 16-K k-step: layer 0 = input_linear o
    # pts_linears.0), su, bias_s, the composed layer 0 (W [256][32] | b [256])
    xfixed = 51 * 1024 * 16 + 2 * 4 * 256 * 4 + 33 * 256 * 4
    zd = 2 * 4096 * 24 * (2 + 4) * 4                   # per-sample (z, segment length), (u, inside)
    # 2 faces = 128 workgroups of 4 tiles: rays split in 2 sample segments, partials of
    # (256 features + rgb, xyz, T, w_last) per segment and ray
    part2 = 2 * (256 + 8) * 2 * 4096 * 4
    assert enc + fixed + xfixed + zd + part2 <= n <= enc + fixed + xfixed + zd + part2 + 1536
    # 1 face = 64 workgroups: 4 sample segments
    n1 = lib.sdfr_render_ngp_workspace_bytes(1, 64, 64, 24, 16)
    part = 4 * (256 + 8) * 4096 * 4
    base1 = enc // 2 + 67 * 1024 * 16 + 8 * 256 * 4 + xfixed + zd // 2
    assert base1 + part <= n1 <= base1 + part + 1536
    n32 = lib.sdfr_render_ngp_workspace_bytes(32, 64, 64, 24, 16)   # >= 256 workgroups: no split
    assert n32 <= 16 * (enc + zd) + fixed + 32 * 8 * 256 * 4 + xfixed + 1536
    # the per-call sample-split bound is validated before anything is launched
    w, a = sdfr._lib.NgpWeights(), sdfr._lib.NgpRenderArgs()
    w.num_levels, a.B, a.H, a.W, a.N = 16, 1, 8, 8, 24
    for bad in (3, 5, 8):
        a.max_field_segments = bad
        assert lib.sdfr_render_ngp_forward(ctypes.byref(w), ctypes.byref(a), None) == \
            sdfr._lib.SDFR_EINVAL
        assert b"max_field_segments" in lib.sdfr_last_error()


def test_conv_split_k_workspace(sdfr):
    """Split-K decisions of the decoder convolutions (host arithmetic, no launch):
    a workspace only when the unsplit grid leaves CUs idle, sized ksplit x slots x one
    128 x 256 fp32 partial tile; the factor is the largest of 4, 3, 2 whose split grid
    stays within 320 workgroups (1.25 rounds of the 256 CUs)."""
    lib = sdfr._lib.lib()
    tile = 16 * 512 * 16
    assert lib.sdfr_conv_ws_bytes(32, 64, 64, 512, 0) == 0            # 2048 workgroups
    assert lib.sdfr_conv_ws_bytes(1, 64, 64, 512, 0) == 4 * 64 * tile  # 64 -> 4 x 64
    assert lib.sdfr_conv_ws_bytes(1, 128, 128, 256, 0) == 2 * 128 * tile
    assert lib.sdfr_conv_ws_bytes(5, 64, 64, 128, 0) == 4 * 80 * tile  # 80 slots: 4-way split
    assert lib.sdfr_conv_ws_bytes(6, 64, 64, 128, 0) == 3 * 96 * tile  # 96 slots: 3-way split
    assert lib.sdfr_conv_act_ws_bytes(1, 64, 64, 512) == lib.sdfr_conv_ws_bytes(1, 64, 64, 512, 0)
    # transposed: four parity classes (17x17, 17x16, 16x17, 16x16 at 16^2), 8-padded
    assert lib.sdfr_conv_ws_bytes(1, 16, 16, 128, 1) == 4 * 32 * tile
    assert lib.sdfr_conv_ws_bytes(1, 64, 64, 256, 1) == 2 * 152 * tile  # 152 slots: 2-way
    assert lib.sdfr_conv_ws_bytes(1, 128, 128, 128, 1) == 0           # 280 slots: no split
    # 32 faces: conv_t_kernel (its edge classes unsplit: splitting them measured slower)
    assert lib.sdfr_conv_ws_bytes(32, 64, 64, 256, 1) == 0
    assert lib.sdfr_conv_ws_bytes(1, 64, 64, 100, 1) == 0             # Cout % 128


def _conv_plan(sdfr, B, H, W, Cin, Cout, transposed, epi, ws=None):
    """sdfr_conv_plan -> (info, [(kernel name, grid x, grid y, block)])."""
    L = sdfr._lib
    q = L.ConvPlanQuery(B, H, W, Cin, Cout, int(transposed), epi, int(ws is not None), ws or 0)
    info = L.ConvPlanInfo()
    assert L.lib().sdfr_conv_plan(ctypes.byref(q), ctypes.byref(info)) == info.rc
    steps = [(L.CONV_PLAN_KERNELS[s.kernel], s.grid_x, s.grid_y, s.block)
             for s in info.steps[:info.nsteps]]
    return info, steps


RAW, STYLED, BLUR = 0, 1, 2
_TILE = 16 * 512 * 16          # one 128 x 256 fp32 partial tile
# (B, H, W, Cin, Cout, transposed, epilogue, conv_t mode, workspace offered) -> launches.
# The decoder's layers (64^2 -> 256^2: styled 256 -> 512, up 512 -> 256, styled 256 -> 256,
# up 256 -> 128, styled 128 -> 128) and a 512 -> 512 styled layer at 1, 4 and 32 faces.
_CONV_PLANS = [
    ((32, 64, 64, 512, 512, 0, STYLED, 1, False), [("conv_h_kernel<false>", 256, 1, 512)]),
    ((4, 64, 64, 512, 512, 0, STYLED, 1, True), [("conv_h_kernel<false>", 256, 1, 512)]),
    ((1, 64, 64, 512, 512, 0, STYLED, 1, True),
     [("conv_h_kernel<true>", 256, 1, 512), ("conv_h_finish_kernel", 64, 4, 128)]),
    ((1, 64, 64, 512, 512, 0, STYLED, 1, False), [("conv_h_kernel<false>", 64, 1, 512)]),
    ((1, 64, 64, 256, 512, 0, STYLED, 1, True),
     [("conv_h_kernel<true>", 256, 1, 512), ("conv_h_finish_kernel", 64, 4, 128)]),
    ((32, 64, 64, 256, 512, 0, STYLED, 1, True), [("conv_h_kernel<false>", 256, 1, 512)]),
    ((1, 128, 128, 256, 256, 0, STYLED, 1, True),
     [("conv_h_kernel<true>", 256, 1, 512), ("conv_h_finish_kernel", 128, 4, 128)]),
    ((4, 128, 128, 256, 256, 0, STYLED, 1, True), [("conv_h_kernel<false>", 256, 1, 512)]),
    ((1, 256, 256, 128, 128, 0, STYLED, 1, True), [("conv_h_kernel<false>", 256, 1, 512)]),
    ((32, 256, 256, 128, 128, 0, STYLED, 1, True), [("conv_h_kernel<false>", 256, 1, 512)]),
    # the upsampling convs, raw output
    ((32, 64, 64, 512, 256, 1, RAW, 1, True),
     [("conv_t_kernel<false>", 256, 1, 512), ("conv_x_kernel<false>", 72, 1, 512)]),
    ((4, 64, 64, 512, 256, 1, RAW, 1, True),
     [("conv_t_kernel<false>", 256, 1, 512), ("conv_x_kernel<false>", 32, 1, 512)]),
    ((1, 64, 64, 512, 256, 1, RAW, 1, True),
     [("conv_x_kernel<false>", 152, 2, 512), ("conv_splitk_kernel<false>", 152, 1, 512)]),
    ((1, 64, 64, 512, 256, 1, RAW, 1, False), [("conv_x_kernel<false>", 152, 1, 512)]),
    ((32, 64, 64, 512, 256, 1, RAW, 0, True), [("conv_x_kernel<false>", 4168, 1, 512)]),
    ((1, 64, 64, 512, 256, 1, RAW, 2, True),
     [("conv_t_kernel<false>", 64, 1, 512), ("conv_x_kernel<false>", 32, 1, 512)]),
    ((1, 64, 64, 512, 256, 1, RAW, 3, True),
     [("conv_t_kernel<false>", 256, 1, 512), ("conv_t_finish_kernel", 4096, 1, 256),
      ("conv_x_kernel<false>", 32, 1, 512)]),
    ((1, 64, 64, 512, 256, 1, RAW, 3, False),
     [("conv_t_kernel<false>", 64, 1, 512), ("conv_x_kernel<false>", 32, 1, 512)]),
    ((32, 128, 128, 256, 128, 1, RAW, 1, True),
     [("conv_t_kernel<false>", 256, 1, 512), ("conv_x_kernel<false>", 72, 1, 512)]),
    ((4, 128, 128, 256, 128, 1, RAW, 1, True),
     [("conv_t_kernel<false>", 256, 1, 512), ("conv_x_kernel<false>", 32, 1, 512)]),
    ((1, 128, 128, 256, 128, 1, RAW, 1, True), [("conv_x_kernel<false>", 280, 1, 512)]),
    # ... and with the blur and the styled epilogue fused (sdfr_conv_t_act)
    ((32, 64, 64, 512, 256, 1, BLUR, 1, False),
     [("conv_t_kernel<true>", 256, 1, 512), ("conv_x_kernel<false>", 72, 1, 512),
      ("conv_t_border_kernel<true>", 1280, 1, 256), ("conv_t_border_kernel<false>", 1280, 1, 256)]),
    ((4, 64, 64, 512, 256, 1, BLUR, 1, False),
     [("conv_t_kernel<true>", 256, 1, 512), ("conv_x_kernel<false>", 32, 1, 512),
      ("conv_t_border_kernel<true>", 160, 1, 256), ("conv_t_border_kernel<false>", 160, 1, 256)]),
    ((32, 128, 128, 256, 128, 1, BLUR, 1, False),
     [("conv_t_kernel<true>", 256, 1, 512), ("conv_x_kernel<false>", 72, 1, 512),
      ("conv_t_border_kernel<true>", 2304, 1, 256), ("conv_t_border_kernel<false>", 2304, 1, 256)]),
    ((1, 64, 64, 512, 256, 1, BLUR, 2, False),
     [("conv_t_kernel<true>", 64, 1, 512), ("conv_x_kernel<false>", 32, 1, 512),
      ("conv_t_border_kernel<true>", 40, 1, 256), ("conv_t_border_kernel<false>", 40, 1, 256)]),
]


@pytest.mark.parametrize("shape,want", _CONV_PLANS)
def test_conv_plan_dispatch(sdfr, shape, want):
    """The launches of the decoder's convolutions (sdfr_conv_plan: host arithmetic, no
    launch): kernel, grid and workgroup size per step, read off the dispatch code; and the
    size queries agree with the plan -- with exactly the reported workspace the plan takes
    its split, with one byte fewer it does not."""
    B, H, W, Cin, Cout, tr, epi, mode, offer = shape
    lib = sdfr._lib.lib()
    prev = lib.sdfr_set_conv_t_mode(mode)
    try:
        free, _ = _conv_plan(sdfr, B, H, W, Cin, Cout, tr, epi)
        assert free.rc == 0 and free.ksplit == 1 and free.ksplit_t == 1
        need = free.ws_bytes
        if epi == STYLED:
            assert lib.sdfr_conv_act_ws_bytes(B, H, W, Cout) == need
        elif epi == RAW:
            assert lib.sdfr_conv_ws_bytes(B, H, W, Cout, tr) == need
        else:
            assert need == 0 and lib.sdfr_conv_t_act_supported(B, H, W, Cin, Cout) == 1
        info, steps = _conv_plan(sdfr, B, H, W, Cin, Cout, tr, epi, need if offer else None)
        assert info.rc == 0 and info.ws_bytes == need
        assert steps == want
        split = info.ksplit * info.ksplit_t
        assert (split > 1) == (offer and need > 0)
        if need:
            short, _ = _conv_plan(sdfr, B, H, W, Cin, Cout, tr, epi, need - 1)
            assert short.rc == 0 and short.ksplit == 1 and short.ksplit_t == 1
    finally:
        lib.sdfr_set_conv_t_mode(prev)


def test_conv_plan_split_factors_and_refusals(sdfr):
    L = sdfr._lib
    lib = L.lib()
    prev = lib.sdfr_set_conv_t_mode(1)
    try:
        info, _ = _conv_plan(sdfr, 1, 64, 64, 512, 512, 0, STYLED, 4 * 64 * _TILE)
        assert (info.ksplit, info.ksplit_t, info.ws_bytes) == (4, 1, 4 * 64 * _TILE)
        info, _ = _conv_plan(sdfr, 1, 64, 64, 512, 256, 1, RAW, 2 * 152 * _TILE)
        assert (info.ksplit, info.ksplit_t, info.ws_bytes) == (2, 1, 2 * 152 * _TILE)
        # 96 channels = 3 groups: conv_h_kernel's split takes whole groups, 4 -> 3
        info, steps = _conv_plan(sdfr, 1, 64, 64, 96, 512, 0, STYLED, 4 * 64 * _TILE)
        assert info.ksplit == 3 and steps[0] == ("conv_h_kernel<true>", 192, 1, 512)
        # H or W not a multiple of 16: the strip kernel carries the styled epilogue
        info, steps = _conv_plan(sdfr, 1, 8, 32, 64, 128, 0, STYLED, 4 * 8 * _TILE)
        assert steps == [("conv_x_kernel<true>", 8, 4, 512), ("conv_splitk_kernel<true>", 8, 1, 512)]
        # below conv_t_kernel's range the fused upsampling conv is refused (mode 1), ...
        info, steps = _conv_plan(sdfr, 1, 64, 64, 512, 256, 1, BLUR)
        assert info.rc == L.SDFR_EUNSUPPORTED and steps == []
        assert b"below conv_t_kernel's range" in lib.sdfr_last_error()
        assert lib.sdfr_conv_t_act_supported(1, 64, 64, 512, 256) == 0
        lib.sdfr_set_conv_t_mode(2)            # ... in mode 2 it is taken at any tile count
        info, _ = _conv_plan(sdfr, 1, 64, 64, 512, 256, 1, BLUR)
        assert info.rc == 0 and lib.sdfr_conv_t_act_supported(1, 64, 64, 512, 256) == 1
        lib.sdfr_set_conv_t_mode(3)            # mode 3: 4 x 129^2 x 256 fp32 partial outputs
        info, _ = _conv_plan(sdfr, 1, 64, 64, 512, 256, 1, RAW, 4 * 129 * 129 * 256 * 4)
        assert (info.ksplit, info.ksplit_t, info.ws_bytes) == (1, 4, 4 * 129 * 129 * 256 * 4)
        assert lib.sdfr_conv_ws_bytes(1, 64, 64, 256, 1) == info.ws_bytes
        # bad channel counts and the 2^31-byte offset limit
        for bad in ((1, 64, 64, 500, 256, 0, RAW), (1, 64, 64, 512, 100, 1, RAW)):
            info, steps = _conv_plan(sdfr, *bad)
            assert info.rc == L.SDFR_EINVAL and steps == [] and b"bad shape" in lib.sdfr_last_error()
        info, _ = _conv_plan(sdfr, 64, 256, 256, 128, 128, 0, STYLED)
        assert info.rc == L.SDFR_EINVAL and b"32-bit offsets" in lib.sdfr_last_error()
        info, _ = _conv_plan(sdfr, 1, 64, 64, 512, 256, 1, STYLED)
        assert info.rc == L.SDFR_EINVAL
    finally:
        lib.sdfr_set_conv_t_mode(prev)


def test_conv_t_act_rejects_misaligned_noise(sdfr):
    """conv_t_kernel<true> reads the noise with 16-B loads: a misaligned pointer is refused
    with the other vector-loaded tensors, before any launch (integers stand in for
    pointers: nothing is dereferenced)."""
    L = sdfr._lib
    lib = L.lib()
    a = L.ConvTActArgs()
    a.x_split, a.packed = 0x10000, 0x20000
    a.B, a.H, a.W, a.Cin, a.Cout = 1, 16, 16, 32, 128
    a.demod, a.bias, a.noise_weight, a.s_next = 0x30000, 0x40000, 0x50000, 0x60000
    a.y_split, a.raw = 0x70000, 0x80000
    a.noise = 0x90000 + 4
    prev = lib.sdfr_set_conv_t_mode(2)
    try:
        assert lib.sdfr_conv_t_act_supported(1, 16, 16, 32, 128) == 1
        assert lib.sdfr_conv_t_act(ctypes.byref(a), None) == L.SDFR_EINVAL
        assert b"16-B aligned" in lib.sdfr_last_error()
    finally:
        lib.sdfr_set_conv_t_mode(prev)


def test_fused_decoder_batch_chunk(sdfr):
    """Faces per fused decoder call (host arithmetic): the largest per-face activation
    of the 64^2 -> 256^2 decoder is the 257^2 x 128 raw output of the last transposed
    convolution, so 63 faces stay under the kernels' 2^31-byte offsets; the split-NHWC
    features the renderer hands over give the same bound."""
    opt = sdfr.vol_render_opt()
    opt.model.feature_encoder_in_channels = opt.rendering.width
    dec = sdfr.Decoder(opt.model)
    seq = [dec.conv1] + list(dec.convs)
    assert dec._fused_chunk(torch.empty(1, 256, 64, 64, device="meta"), seq) == 63
    assert dec._fused_chunk(torch.empty(1, 64, 64, 32, 2, 8, device="meta"), seq) == 63
    assert (2 ** 31 - 1) // (257 * 257 * 128 * 4) == 63


def test_state_dict_matches_reference(sdfr, golden_dir):
    opt = sdfr.vol_render_opt()
    g = sdfr.Generator(opt.model, opt.rendering)
    mine = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    ref = dict(W.golden_entries(golden_dir))
    assert mine == ref


def test_siren_state_dict_matches_reference(sdfr, golden_dir):
    opt = sdfr.vol_render_opt(ngp=False)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False)
    mine = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    assert mine == dict(W.golden_entries(golden_dir, siren=True))


def test_seeded_init_identical_to_reference(sdfr, golden_dir):
    z = np.load(golden_dir / "init_stats.npz")
    opt = sdfr.vol_render_opt()
    torch.manual_seed(0)
    g = sdfr.Generator(opt.model, opt.rendering)
    sd = g.state_dict()
    for k, st in zip(z["names"], z["stats"]):
        v = sd[str(k)].double().reshape(-1)
        mine = [v.sum().item(), (v * v).sum().item(), v[0].item(), v[-1].item()]
        np.testing.assert_allclose(mine, st, rtol=1e-12, atol=1e-12, err_msg=str(k))
    assert [k for k, _ in g.named_parameters()] == list(z["param_order"])


def test_camera_matches_reference(sdfr, golden_dir):
    g = np.load(golden_dir / "camera.npz")
    for name, kw in [("gauss", {}), ("uniform", {"uniform": True}), ("sweep", {"sweep": True})]:
        torch.manual_seed(123)
        out = sdfr.generate_camera_params(64, "cpu", batch=5, **kw)
        for k, v in zip(["ext", "focal", "near", "far", "vp"], out):
            np.testing.assert_array_equal(v.numpy(), g[f"{name}_{k}"], err_msg=f"{name}_{k}")
    locs = torch.from_numpy(g["loc_locations"])
    out = sdfr.generate_camera_params(128, "cpu", batch=locs.shape[0], locations=locs)
    for k, v in zip(["ext", "focal", "near", "far", "vp"], out):
        np.testing.assert_array_equal(v.numpy(), g[f"loc_{k}"])


@pytest.fixture(scope="module")
def det_generator(sdfr):
    opt = sdfr.vol_render_opt()
    g = sdfr.Generator(opt.model, opt.rendering)
    W.det_init_(g)
    return g.eval()


def test_decoder_matches_reference(det_generator, golden_dir):
    z = np.load(golden_dir / "generator.npz")
    with torch.no_grad():
        img, _ = det_generator.decoder(torch.from_numpy(z["dec_feats"]),
                                       [torch.from_numpy(z["dec_latent"])],
                                       randomize_noise=False)
    # batched modulation conv(x*s, W)*demod vs the reference's per-face weights
    np.testing.assert_allclose(img.numpy(), z["dec_img"], rtol=0, atol=2e-5)


def test_mapping_and_mean_latent(det_generator, golden_dir):
    z = np.load(golden_dir / "generator.npz")
    with torch.no_grad():
        lat = det_generator.style(torch.from_numpy(z["z"]))
        np.testing.assert_array_equal(lat.numpy(), z["dec_latent"])
        mean = det_generator.mean_latent(64, "cpu", z=torch.from_numpy(z["mean_z"]))
    np.testing.assert_array_equal(mean[0].numpy(), z["mean_renderer"])
    np.testing.assert_array_equal(mean[1].numpy(), z["mean_decoder"])


def test_cpu_tensors_rejected_like_reference(sdfr):
    enc = sdfr.GridEncoder(desired_resolution=4096)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        enc(torch.zeros(4, 3), bound=2)
    sh = sdfr.SHEncoder()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sh(torch.zeros(4, 3))


def test_options_defaults(sdfr):
    opt = sdfr.vol_render_opt()
    assert opt.rendering.N_samples == 24 and opt.rendering.perturb == 1.0
    assert opt.model.renderer_spatial_output_dim == 64 and opt.model.size == 256
    assert opt.camera.fov == 6 and opt.camera.dist_radius == 0.12
    assert opt.rendering.type == "ngp" and opt.model.freeze_renderer
    o1 = sdfr.vol_render_opt(train_renderer=True)
    assert "no_features_output" in o1.rendering and o1.rendering.return_sdf


def test_fused_path_selection(sdfr):
    opt = sdfr.vol_render_opt()
    r = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=8)
    cam = torch.zeros(1, 3, 4)
    st = torch.zeros(1, 256)
    with torch.no_grad():
        assert not r._fused_ok(cam, st, False)      # CPU tensors never take the HIP path
    opt2 = sdfr.vol_render_opt(ngp=False)
    r2 = sdfr.VolumeFeatureRenderer(opt2.rendering, style_dim=256, out_im_res=8)
    assert isinstance(r2.network, sdfr.SirenGenerator)


def test_align_volume_matches_reference(sdfr, golden_dir):
    """sdf_utils.align_volume on a random volume: same grid_sample, bit for bit."""
    g = np.load(golden_dir / "mesh128.npz")
    out = sdfr.align_volume(torch.from_numpy(g["vol"]))
    np.testing.assert_array_equal(out.numpy(), g["vol_aligned"])


def test_xyz2mesh_faces(sdfr):
    xyz = torch.arange(3 * 4 * 5, dtype=torch.float32).reshape(1, 3, 4, 5)
    res = sdfr.xyz2mesh(xyz)
    verts, faces = res if isinstance(res, tuple) else (res.vertices, res.faces)
    assert verts.shape == (20, 3) and faces.shape[1] == 3 and faces.max() < 20


def test_graphed_generator_rejects_cpu(sdfr):
    opt = sdfr.vol_render_opt()
    g = sdfr.Generator(opt.model, opt.rendering).eval()
    with pytest.raises(RuntimeError, match="on a GPU"):
        sdfr.GraphedGenerator(g)


def test_get_rays_bit_exact_vs_reference(sdfr, golden_dir):
    """get_rays' rays_d as the explicit left-to-right sum equals the reference's
    torch.sum (sdf_model.py:213) on CPU, bit for bit (the GPU test repeats it on cuda)."""
    g = np.load(golden_dir / "render_small.npz")
    opt = sdfr.vol_render_opt()
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=int(g["res"]))
    _, rays_d, viewdirs = ren.get_rays(torch.from_numpy(g["focal"]), torch.from_numpy(g["ext"]))
    np.testing.assert_array_equal(rays_d.numpy(), g["rays_d"])
    vd = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
    np.testing.assert_array_equal(vd.numpy(), g["viewdirs"])


def _golden_renderer(sdfr, golden_dir, name, kind):
    g = np.load(golden_dir / f"{name}.npz")
    opt = sdfr.vol_render_opt(ngp=kind == "ngp", fc=kind == "fc")
    r = opt.rendering
    r.N_samples = int(g["n_samples"])
    for k, v in ast.literal_eval(str(g["render_opts"])).items():   # the fixture's options
        if k in ("return_sdf", "return_xyz", "static_viewdirs", "force_background", "perturb"):
            r[k] = v
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=int(g["res"]))
    amp = float(g["table_amp"]) if "table_amp" in g.files else 1.0
    sd = W.det_state_dict(W.golden_entries(golden_dir, kind=kind), "renderer.", table_amp=amp)
    ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()}, strict=True)
    return g, ren.eval()


def test_fc_state_dict_matches_reference(sdfr, golden_dir):
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False)
    mine = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    assert mine == dict(W.golden_entries(golden_dir, kind="fc"))


def test_fc_renderer_matches_reference_cpu(sdfr, golden_dir):
    """rendering.fc = 1 (FCGenerator, sdf_model.py:1599-1670): the drop-in renderer on
    CPU runs the reference's torch ops in the reference's order."""
    g, ren = _golden_renderer(sdfr, golden_dir, "render_fc_small", "fc")
    assert isinstance(ren.network, sdfr.FCGenerator)
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    with torch.no_grad():
        rgb, feat, sdf, mask, xyz, _ = ren(t("ext"), t("focal"), t("near"), t("far"),
                                           styles=t("latent"), t_rand=t("t_rand"))
    for k, v in dict(rgb=rgb, features=feat, sdf=sdf, xyz=xyz, mask=mask).items():
        np.testing.assert_allclose(v.numpy(), g[k], rtol=0, atol=1e-6, err_msg=k)

"""CPU: the fused decoder's plan (decoder_fused.DecoderPlan) -- the style layout handed to
sdfr_decoder_styles, the stacked modulation weights and the routing of every layer."""
import copy
import itertools
import pickle

import pytest
import torch


def _decoder(sdfr, size=256, style_dim=None, in_feat=None):
    opt = sdfr.vol_render_opt()
    opt.model.feature_encoder_in_channels = in_feat or opt.rendering.width
    opt.model.size = size
    if style_dim is not None:
        opt.model.style_dim = style_dim
    torch.manual_seed(size)
    return sdfr.Decoder(opt.model)


def _layout(dec):
    """Latent index and width per stacked layer from ``channels`` and the layer order:
    conv1, then (upsampling conv, conv) per octave; then to_rgb1 and one ToRGB per octave.
    Conv i reads latent i, ToRGB k latent 2k + 1."""
    res = [2 ** r for r in range(dec.log_in_size, dec.log_size + 1)]
    ch = [dec.channels[r] for r in res]
    conv_in = [dec.conv1.conv.in_channel]
    for a, b in zip(ch, ch[1:]):
        conv_in += [a, b]
    n = len(conv_in)
    return list(range(n)) + [2 * k + 1 for k in range(len(ch))], conv_in + ch


@pytest.mark.parametrize("size", [256, 1024])
def test_style_layout(sdfr, size):
    dec = _decoder(sdfr, size)
    plan = dec._fused_plan().load()
    index, widths = _layout(dec)
    if size == 256:
        assert index == [0, 1, 2, 3, 4, 1, 3, 5]
        assert widths == [256, 512, 256, 256, 128, 512, 256, 128]
        assert dec.n_latent == 6
    else:
        assert len(index) == 14 and dec.n_latent == 10
    assert plan.mod_index == index and plan.mod_c == widths
    assert max(index) == dec.n_latent - 1
    L, a = len(index), plan.style_args
    assert (a.L, a.K, a.cmax) == (L, 512, 512)
    assert list(a.mod_index[:L]) == index and list(a.mod_c[:L]) == widths
    for B in (1, 3):
        offs, total = plan._offsets(B, plan.mod_c)
        assert offs == [B * sum(widths[:k]) for k in range(L)]
        assert total == B * sum(widths)
    # a copied or pickled decoder starts without a plan; nothing of a plan is a parameter
    # or buffer
    assert copy.deepcopy(dec)._plan is None and pickle.loads(pickle.dumps(dec))._plan is None
    assert not any("plan" in k for k in dec.state_dict())


def test_stacked_modulation_weights_reproduce_the_modules(sdfr):
    """latent[:, idx_k] @ mw[k, :c].T + mb[k, :c] in float64 equals modulation_k of the fp32
    module to the module GEMM's rounding: (K + 2) 2^-24 (sum |x w| + |b|) per element.  Both
    sides start from the same fp32 ``weight * scale`` and ``bias * lr_mul``; the module then
    rounds a K-term dot product and the bias add in fp32 (at most K + 1 roundings on any
    summation path, whatever the GEMM's order, first order in 2^-24; one to spare)."""
    dec = _decoder(sdfr)
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, sdfr.EqualLinear):
                m.bias.normal_(1, 0.5)
    plan = dec._fused_plan().load()
    g = torch.Generator().manual_seed(1)
    latent = torch.randn(3, dec.n_latent, 512, generator=g)
    K = 512
    for k, m in enumerate(plan.lins):
        c = plan.mod_c[k]
        x = latent[:, plan.mod_index[k]]
        with torch.no_grad():
            want = m(x).double()
        w, b = plan.mod_w[k, :c].double(), plan.mod_b[k, :c].double()
        got = x.double() @ w.t() + b
        bound = (K + 2) * 2.0 ** -24 * (x.double().abs() @ w.abs().t() + b.abs())
        assert got.shape == want.shape == (3, c)
        assert bool(((got - want).abs() <= bound).all()), k
        assert not plan.mod_w[k, c:].any() and not plan.mod_b[k, c:].any()     # zero padding


# The route of every layer, written out per (size, fuse_conv_act, fuse_conv_t_blur) for
# conv_impl = "f16x3" (with "miopen" every layer is M).  A conv_act, S split_conv+epilogue,
# M miopen+epilogue; T is conv_t_act where sdfr_conv_t_act_supported takes the shape (4 faces:
# 256 tiles and more) and S where it does not (1 face).  From the four rules: conv_act needs
# fuse_conv_act, a regular split layer, a pixel count that is a multiple of 256 and a split
# next layer (or none); conv_t_act needs fuse_conv_t_blur, an upsampling split layer with
# i % 2 == 1 and a split next layer.  The 1024^2 decoder's layers 5-8 have 64 / 32 channels
# and are not split: layer 4 (split, regular) is followed by a non-split one and stays S with
# conv_act on, and the last layer is M.
ROUTES = {
    (256, True, True): "ATATA", (256, True, False): "ASASA",
    (256, False, True): "STSTS", (256, False, False): "SSSSS",
    (1024, True, True): "ATATSMMMM", (1024, True, False): "ASASSMMMM",
    (1024, False, True): "STSTSMMMM", (1024, False, False): "SSSSSMMMM",
}
NAMES = {"A": "conv_act", "T": "conv_t_act", "S": "split_conv+epilogue", "M": "miopen+epilogue"}


@pytest.mark.parametrize("size", [256, 1024])
def test_routes(sdfr, size):
    dec = _decoder(sdfr, size)
    lib = sdfr._lib.lib()
    seen = set()
    for conv_impl, fuse_act, fuse_t, B in itertools.product(
            ("f16x3", "miopen"), (True, False), (True, False), (1, 4)):
        dec.conv_impl, dec.fuse_conv_act, dec.fuse_conv_t_blur = conv_impl, fuse_act, fuse_t
        plan = dec._fused_plan()
        table = ROUTES[size, fuse_act, fuse_t] if conv_impl == "f16x3" else "M" * len(plan.layers)
        assert [ly.split for ly in plan.layers] == [c != "M" for c in table]
        got, want, H = [], [], 64
        for i, (ly, c) in enumerate(zip(plan.layers, table, strict=True)):
            got.append(plan.route(i, B, H, H, fuse_act, fuse_t))
            if c == "T":
                ok = bool(lib.sdfr_conv_t_act_supported(B, H, H, ly.cin, ly.cout))
                assert ok == (B == 4)
                c = "T" if ok else "S"
            want.append(NAMES[c])
            H = 2 * H if ly.upsample else H
        assert got == want, (conv_impl, fuse_act, fuse_t, B)
        seen.update(got)
    assert seen == set(NAMES.values())


def test_unsupported_latent_width_is_not_fused_ready(sdfr):
    """style_dim 64 gives a latent width of 128, which sdfr_decoder_styles does not take:
    the decoder-only half of the check says so (no tensor, no GPU), and forward() then runs
    the module path."""
    dec = _decoder(sdfr, style_dim=64)
    assert dec.style_dim == 128
    assert not dec._fused_plan().supported
    with torch.no_grad():
        assert dec.fused_ready(torch.device("cuda", 0)) is False
    # ... nor a modulation wider than 512 (768 feature channels into conv1)
    wide = _decoder(sdfr, in_feat=768)
    assert wide._fused_plan().cmax == 768 and not wide._fused_plan().supported
    # ... nor modulation weights that are not fp32
    assert not _decoder(sdfr).double()._fused_plan().supported
    ok = _decoder(sdfr)
    assert ok._fused_plan().supported
    with torch.no_grad():
        assert ok.fused_ready(torch.device("cuda", 0)) is True
        assert ok.fused_ready(torch.device("cpu")) is False

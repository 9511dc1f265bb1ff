"""What the decoder's two HIP-backed autograd ops (sdface-gan_amd/decoder_ops.py:
``fused_leaky_relu`` on sdfr_fused_bias_act, ``upfirdn2d`` on sdfr_upfirdn2d) are held to,
first and second order, and the two losses that differentiate twice through them
(training.d_r1_loss, training.g_path_regularize).  Test infrastructure; the product never
falls back to it.  Device- and dtype-agnostic: every result lives where its inputs live.

  native_fused_leaky_relu, native_upfirdn2d, upfirdn2d_native
        the reference's PyTorch formulas (sdf_op.py:106-114, :273-316) with the call
        signatures of decoder_ops.fused_leaky_relu / upfirdn2d; torch autograd differentiates
        them, to any order
  standin_fused_bias_act, standin_upfirdn2d_op
        plain torch restatements of the two library calls' contracts (include/sdfr.h),
        detached like a kernel's output: with them the custom Functions run on CPU tensors
        in float64, which checks their ctx plumbing and pad arithmetic without a GPU
  function_fused_leaky_relu, function_upfirdn2d
        the ``Function.apply`` forms, whatever the device (decoder_ops routes CPU tensors
        to the native formulas)
  MiniD, MiniG, mini_d, mini_g
        small stacks of the project's own discriminator / decoder modules
  r1_grads, path_grads
        the two losses and their gradients with respect to every parameter
  recording()
        every leaky ReLU seen while it is open: min |x + bias| and the activation
"""
import contextlib
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import autograd

from sdfr_loader import load

sdfr = load()
ops = sdfr.decoder_ops
gen = sdfr.generator
training = sdfr.training
upfirdn2d_native = ops.upfirdn2d_native

BLUR = (1.0, 3.0, 3.0, 1.0)

# (up, down, pad) of the modules that call upfirdn2d with the 4x4 blur taps: Upsample
# (generator.py:52), the upsampling ModulatedConv2d's Blur (:177), the discriminator's
# Blur before a strided 3x3 / 1x1 convolution (training.py:55)
MODULE_PADS = [(2, 1, (2, 1)), (1, 1, (1, 1)), (1, 1, (2, 2))]

# tiled kernel (upfirdn2d_tile_kernel: 64 output columns x 32 rows, 16 when down = 2):
# input shape, up, down, pad; forward or backward of each crosses a tile edge on both axes
TILE_CASES = [((2, 3, 40, 72), 1, 1, (2, 2)), ((2, 3, 40, 72), 1, 1, (1, 1)),
              ((1, 2, 20, 36), 2, 1, (2, 1)), ((1, 2, 41, 73), 1, 2, (2, 2))]
# generic kernel (upfirdn2d_kernel): random, asymmetric taps of these shapes on (2,2,13,17)
GENERIC_CASES = [(2, 2, (-1, 3), (3, 5)), (3, 1, (0, 0), (2, 2))]


def blur_taps(up=1, dtype=torch.float32):
    f = torch.tensor(BLUR, dtype=dtype)
    k = torch.outer(f, f)
    return k / k.sum() * (up * up)


# ---------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------
_rec = None


@contextlib.contextmanager
def recording():
    """Collects, per leaky ReLU evaluated while open, {"min_abs": min |x + bias|,
    "out": the activation as float64 on the CPU}."""
    global _rec
    prev, _rec = _rec, []
    try:
        yield _rec
    finally:
        _rec = prev


def _note(pre, out):
    if _rec is not None:
        _rec.append({"min_abs": float(pre.detach().abs().min()),
                     "out": out.detach().double().cpu()})


def _with_bias(x, bias):
    if bias is None or bias.numel() == 0:
        return x
    return x + bias.view(1, -1, *([1] * (x.ndim - 2)))


# ---------------------------------------------------------------------------
# native formulas
# ---------------------------------------------------------------------------
def native_fused_leaky_relu(input, bias=None, negative_slope=0.2, scale=2 ** 0.5):
    v = _with_bias(input, bias)
    out = F.leaky_relu(v, negative_slope=negative_slope) * scale
    _note(v, out)
    return out


def native_upfirdn2d(input, kernel, up=1, down=1, pad=(0, 0)):
    return upfirdn2d_native(input, kernel, up, up, down, down, pad[0], pad[1], pad[0], pad[1])


# ---------------------------------------------------------------------------
# stand-ins for the library calls
# ---------------------------------------------------------------------------
def standin_fused_bias_act(input, bias, refer, act, grad, alpha, scale):
    """sdfr_fused_bias_act for the leaky ReLU (act 3): out = f(x + bias[c]) * scale with
    f(t) = t > 0 ? t : t alpha (grad 0: mode 30) or ref > 0 ? t : t alpha (grad 1: mode
    31); bias indexed along dim 1 and, like ``refer``, possibly empty; contiguous output."""
    assert act == 3 and grad in (0, 1)
    t = _with_bias(input.detach().contiguous(), None if bias is None else bias.detach())
    if grad == 0:
        sel = t
    else:
        assert refer is not None and refer.shape == input.shape
        sel = refer.detach().contiguous()
    return (torch.where(sel > 0, t, t * alpha) * scale).detach()


def standin_upfirdn2d_op(x, kernel, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """sdfr_upfirdn2d: x [major, h, w] -> [major, out_h, out_w]."""
    major, h, w = x.shape
    out = upfirdn2d_native(x.detach().reshape(major, 1, h, w), kernel.detach(), up_x, up_y,
                           down_x, down_y, px0, px1, py0, py1)
    return out.reshape(major, out.shape[2], out.shape[3]).detach()


# ---------------------------------------------------------------------------
# the Function.apply forms
# ---------------------------------------------------------------------------
def function_fused_leaky_relu(input, bias=None, negative_slope=0.2, scale=2 ** 0.5):
    out = ops.FusedLeakyReLUFunction.apply(input, bias, negative_slope, scale)
    if _rec is not None:
        with torch.no_grad():
            _note(_with_bias(input, bias), out)
    return out


def function_upfirdn2d(input, kernel, up=1, down=1, pad=(0, 0)):
    return ops.UpFirDn2d.apply(input, kernel, (up, up), (down, down),
                               (pad[0], pad[1], pad[0], pad[1]))


def route(monkeypatch, fused_leaky_relu, upfirdn2d):
    """Point the three module globals through which the project's modules reach the two
    ops (FusedLeakyReLU: decoder_ops.fused_leaky_relu; EqualLinear: generator.
    fused_leaky_relu; Blur / Upsample: generator.upfirdn2d) at the given functions."""
    monkeypatch.setattr(ops, "fused_leaky_relu", fused_leaky_relu)
    monkeypatch.setattr(gen, "fused_leaky_relu", fused_leaky_relu)
    monkeypatch.setattr(gen, "upfirdn2d", upfirdn2d)


def route_native(monkeypatch):
    route(monkeypatch, native_fused_leaky_relu, native_upfirdn2d)


def route_functions(monkeypatch):
    route(monkeypatch, function_fused_leaky_relu, function_upfirdn2d)


def route_standins(monkeypatch):
    """The custom Functions on the stand-ins: they then run on any device and dtype."""
    monkeypatch.setattr(ops, "fused_bias_act", standin_fused_bias_act)
    monkeypatch.setattr(ops, "_upfirdn2d_op", standin_upfirdn2d_op)
    route_functions(monkeypatch)


# ---------------------------------------------------------------------------
# the two stacks
# ---------------------------------------------------------------------------
STYLE_DIM = 32


class MiniD(nn.Module):
    """The discriminator's layer kinds (training.py:80-117) at 8 / 16 channels: 1x1
    ConvLayer, two downsampling ResBlocks (Blur pads (2,2) and (1,1)), the 2-D
    fused_lrelu EqualLinear and the output EqualLinear."""

    def __init__(self, height, width):
        super().__init__()
        self.convs = nn.Sequential(training.ConvLayer(3, 8, 1), training.ResBlock(8, 16),
                                   training.ResBlock(16, 16))
        self.final_linear = nn.Sequential(
            gen.EqualLinear(16 * (height // 4) * (width // 4), 16, activation="fused_lrelu"),
            gen.EqualLinear(16, 1))

    def forward(self, input):
        out = self.convs(input)
        return self.final_linear(out.view(out.shape[0], -1))


class MiniG(nn.Module):
    """The decoder's layer kinds with its latent indexing (generator.py:538-548): a
    StyledConv and ToRGB at the input size, one upsampling block (transposed conv + Blur
    (1,1), StyledConv, ToRGB with the skip through Upsample)."""

    def __init__(self):
        super().__init__()
        self.conv1 = gen.StyledConv(8, 16, 3, STYLE_DIM)
        self.to_rgb1 = gen.ToRGB(16, STYLE_DIM, upsample=False)
        self.up = gen.StyledConv(16, 8, 3, STYLE_DIM, upsample=True)
        self.conv2 = gen.StyledConv(8, 8, 3, STYLE_DIM)
        self.to_rgb = gen.ToRGB(8, STYLE_DIM)

    def forward(self, feat, latent, noises):
        out = self.conv1(feat, latent[:, 0], noise=noises[0])
        skip = self.to_rgb1(out, latent[:, 1])
        out = self.up(out, latent[:, 1], noise=noises[1])
        out = self.conv2(out, latent[:, 2], noise=noises[2])
        return self.to_rgb(out, latent[:, 3], skip=skip)


def _perturb(model, g):
    """Biases + N(0, 0.3), noise weights 0.3: no term of either op's backward is zero."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.rsplit(".", 1)[-1] == "bias":
                p.add_(torch.randn(p.shape, generator=g) * 0.3)
        for m in model.modules():
            if isinstance(m, gen.NoiseInjection):
                m.weight.fill_(0.3)
    return model


def _seeded(make, seed):
    g = torch.Generator().manual_seed(seed)
    state = torch.get_rng_state()
    try:
        torch.manual_seed(seed)            # the modules draw their weights from the global RNG
        model = make()
    finally:
        torch.set_rng_state(state)
    return _perturb(model, g), g


D_SHAPE = (2, 3, 12, 20)
G_FEAT, G_LATENT = (2, 8, 6, 10), (2, 4, STYLE_DIM)
G_NOISES = [(2, 1, 6, 10), (2, 1, 12, 20), (2, 1, 12, 20)]


def mini_d(seed, shape=D_SHAPE):
    """(MiniD, x) in fp32 on the CPU; other precisions and devices are copies of these."""
    model, g = _seeded(lambda: MiniD(shape[2], shape[3]), seed)
    return model, torch.randn(shape, generator=g)


def mini_g(seed, scale=1):
    """(MiniG, feat, w, noises, pl_noise) in fp32 on the CPU; ``scale`` multiplies the
    feature size (1: 6 x 10 -> 12 x 20)."""
    model, g = _seeded(MiniG, seed)
    sz = lambda s: s[:2] + (s[2] * scale, s[3] * scale)      # noqa: E731
    feat = torch.randn(sz(G_FEAT), generator=g)
    w = torch.randn(G_LATENT, generator=g)
    noises = [torch.randn(sz(s), generator=g) for s in G_NOISES]
    pl_noise = torch.randn((2, 3) + sz(G_NOISES[-1])[2:], generator=g)
    return model, feat, w, noises, pl_noise


def cast(model, *tensors, device="cpu", dtype=torch.float32):
    """A copy of the model and of each tensor (lists of tensors too) on device / dtype."""
    to = lambda t: ([to(u) for u in t] if isinstance(t, (list, tuple))      # noqa: E731
                    else t.detach().to(device=device, dtype=dtype))
    return (copy.deepcopy(model).to(device=device, dtype=dtype),) + tuple(to(t) for t in tensors)


# ---------------------------------------------------------------------------
# the two loss gradients
# ---------------------------------------------------------------------------
def _param_grads(loss, model):
    names, params = zip(*model.named_parameters())
    grads = autograd.grad(loss, params, allow_unused=True)
    return dict(zip(names, grads))


def r1_grads(model, x):
    """training.d_r1_loss on model(x): (loss, {parameter name: gradient or None})."""
    x = x.detach().requires_grad_(True)
    loss = training.d_r1_loss(model(x), x)
    return loss.detach(), _param_grads(loss, model)


class _FixedNoise:
    """The torch module as training.py sees it, with randn_like returning a given draw."""

    def __init__(self, noise):
        self._noise = noise

    def randn_like(self, t):
        assert t.shape == self._noise.shape
        return self._noise.to(device=t.device, dtype=t.dtype)

    def __getattr__(self, name):
        return getattr(torch, name)


def path_grads(model, feat, w, noises, pl_noise, mean_path_length=0.5):
    """training.g_path_regularize on model(feat, w, noises) with ``pl_noise`` as the draw
    of its torch.randn_like (``None``: its own draw): (penalty, path lengths, {parameter
    name: gradient of the penalty or None})."""
    w = w.detach().requires_grad_(True)
    img = model(feat, w, noises)
    prev = training.torch
    if pl_noise is not None:
        training.torch = _FixedNoise(pl_noise)
    try:
        penalty, _, lengths = training.g_path_regularize(img, w, mean_path_length)
    finally:
        training.torch = prev
    return penalty.detach(), lengths.detach(), _param_grads(penalty, model)


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def rel_err(got, ref):
    """max |got - ref| / max |ref| in float64 on the CPU; ``None`` counts as zero.  For a
    reference that is exactly zero (or None): 0.0 if got is None or exactly zero, else inf."""
    r = None if ref is None else ref.detach().double().cpu()
    g = None if got is None else got.detach().double().cpu()
    if r is None or not bool(r.any()):
        return 0.0 if g is None or not bool(g.any()) else float("inf")
    if g is None:
        g = torch.zeros_like(r)
    assert g.shape == r.shape, (g.shape, r.shape)
    return float((g - r).abs().max() / r.abs().max())


def is_zero(t):
    return t is None or not bool(t.any())

"""GPU: first- and second-order gradients of the decoder's two HIP-backed ops
(decoder_ops.fused_leaky_relu on sdfr_fused_bias_act, decoder_ops.upfirdn2d on
sdfr_upfirdn2d) against float64, and the two losses of stage-2 training that differentiate
twice through them (d_r1_loss, g_path_regularize) through small stacks of the project's
modules (tests/decoder_autograd_ref.py).

fused_bias_act is element-wise in a fixed operation order: forward, grad_x and the
double-backward term are BIT-EXACT against that order evaluated in fp32; grad_bias (a
torch.sum of the kernel's output) is held to 4 x the error of a CPU fp32 sum of the same
terms.  upfirdn2d sums its taps in another order than the float64 formula: 1e-5 absolute
on O(1) data with normalised taps (tests/test_gpu_decoder.py's bound); its second-order
term is the forward kernel itself.  The losses' gradients are held to 4 x the error that
PyTorch's own ops make in fp32 on the same formula (CPU and GPU), relative to max |ref|,
with every leaky ReLU proven to be on the float64 reference's branch.  Every measured
figure goes to the parity JSON (profiles/decoder_autograd_parity.json).  Measured on an
MI355X: grad_bias <= 0.25 of its bound; upfirdn2d <= 5.2e-7 in all three orders; loss
gradients <= 1.2e-6 of max |ref| against bars of 1.8e-6 ... 5.1e-6 (at most 0.29 of the
bar); activations within 1.3e-6 max(1, |ref|) of the reference's, kink margins >= 1.7e-4.
"""
import json
import math
import os

import pytest
import torch
from torch import autograd

from tests import decoder_autograd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
_record = {}


def teardown_module(module):
    out = os.environ.get("SDFR_PARITY_JSON")
    if out:
        with open(out.replace(".json", "_decoder_autograd.json"), "w") as f:
            json.dump(_record, f, indent=1, sort_keys=True)


def _close(name, got, ref, atol):
    err = float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max())
    _record[name] = err
    print(f"{name}: max err {err:.3e}")
    assert got.shape == ref.shape
    assert err <= atol, f"{name}: max err {err:.3e} > {atol:.1e}"


# ---------------------------------------------------------------------------
# fused_leaky_relu
# ---------------------------------------------------------------------------
ALPHA, SCALE = 0.2, math.sqrt(2)


def _takes_vec_kernel(shape, with_bias):
    """sdfr_fused_bias_act's choice (csrc/decoder.hip): the float4 kernel when the element
    count and, with a bias, the bias step are multiples of 4 (torch's allocations are
    16-byte aligned)."""
    return math.prod(shape) % 4 == 0 and (not with_bias or math.prod(shape[2:]) % 4 == 0)


# shape, with_bias, float4 kernel?  (the expectation is checked against the rule above)
FLR = [((3, 16, 9, 9), True, False),       # step_b = 81: scalar kernel
       ((3, 16, 9, 9), False, True),
       ((2, 8, 8, 12), True, True),        # step_b = 96: float4 kernel, 24 float4 per bias entry
       ((2, 8, 8, 12), False, True),
       ((5, 24), True, False),             # 2-D (EqualLinear fused_lrelu): step_b = 1
       ((5, 24), False, True),
       ((4, 32), True, False),
       ((4, 32), False, True),
       ((1, 3, 64, 257), True, True),      # step_b = 16448 = 4 x 4112, 49 blocks of 256 float4
       ((1, 3, 64, 257), False, True),
       ((1, 3, 63, 257), True, False),     # odd element count: scalar kernel, 190 blocks
       ((1, 3, 63, 257), False, False)]


def _lrelu32(sel, t):
    """where(sel > 0, t, t alpha) scale in fp32 on the CPU: the kernel's operation order,
    alpha and scale rounded to fp32 as the kernel receives them."""
    a, s = torch.tensor(ALPHA, dtype=torch.float32), torch.tensor(SCALE, dtype=torch.float32)
    return torch.where(sel > 0, t, t * a) * s


def _noncontiguous(x):
    if x.ndim == 4:
        return x.contiguous(memory_format=torch.channels_last)
    return x.t().contiguous().t()


@pytest.mark.parametrize("shape,with_bias,vec", FLR)
def test_fused_leaky_relu_first_and_second_order(shape, with_bias, vec):
    assert _takes_vec_kernel(shape, with_bias) == vec
    ops = R.ops
    g = torch.Generator().manual_seed(sum(shape) + with_bias)
    r = torch.randn(shape, generator=g)
    x = torch.sign(r) * (r.abs() + 0.01)            # no pre-activation within 5e-3 of the kink
    b = (torch.rand(shape[1], generator=g) * 2 - 1) * 0.005 if with_bias else None
    go, v = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    u = torch.randn(shape[1], generator=g)
    bview = (1, -1) + (1,) * (len(shape) - 2)
    pre = x + b.view(bview) if with_bias else x
    assert float(pre.abs().min()) >= 5e-3
    tag = f"flrelu_{'x'.join(map(str, shape))}_{'bias' if with_bias else 'nobias'}"

    xg = x.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True) if with_bias else None
    gog = go.to(DEV).requires_grad_(True)
    ins = (xg, bg) if with_bias else (xg,)
    out = ops.fused_leaky_relu(xg, bg)
    first = autograd.grad(out, ins, gog, create_graph=True)
    second = (first[0] * v.to(DEV)).sum()
    if with_bias:
        second = second + (first[1] * u.to(DEV)).sum()
    gg = autograd.grad(second, (gog,) + ins, allow_unused=True)
    torch.cuda.synchronize()

    # (a) forward, (b) grad_x: bit-equal to the fp32 formula in the kernel's order
    out_ref = _lrelu32(pre, pre)
    assert torch.equal(out.detach().cpu(), out_ref)
    gx_ref = _lrelu32(out_ref, go)
    assert torch.equal(first[0].detach().cpu(), gx_ref)
    # (c) grad_bias against the float64 sum of the same fp32 terms
    if with_bias:
        dims = [0] + list(range(2, len(shape)))
        exact = gx_ref.double().sum(dims)
        err = (first[1].detach().double().cpu() - exact).abs()
        err_cpu = (gx_ref.sum(dims).double() - exact).abs()
        floor = 2.0 ** -23 * gx_ref.double().abs().sum(dims)
        bound = torch.maximum(4 * err_cpu, floor)
        _record[tag + "_grad_bias"] = {"err": float(err.max()), "cpu_fp32_sum_err":
                                       float(err_cpu.max()), "floor": float(floor.min()),
                                       "err_over_bound": float((err / bound).max())}
        print(tag, _record[tag + "_grad_bias"])
        assert first[1].shape == (shape[1],) and bool((err <= bound).all())
    # (d) second order: fused_bias_act(v, u, ref = out) in mode 31, bias path included
    t = v + u.view(bview) if with_bias else v
    assert torch.equal(gg[0].cpu(), _lrelu32(out_ref, t))
    for extra in gg[1:]:
        assert R.is_zero(extra)                      # piecewise linear in x and the bias
    _record[tag + "_bit_exact"] = ["forward", "grad_x", "gradgrad_go"]

    # (e) a stride-0 grad_output and a non-contiguous input give the contiguous call's bits
    def first_order(xin, grad_out):
        xi = xin.detach().requires_grad_(True)
        bi = bg.detach().requires_grad_(True) if with_bias else None
        o = ops.fused_leaky_relu(xi, bi)
        if grad_out is None:
            o.sum().backward()
        else:
            o.backward(grad_out)
        return o.detach(), xi.grad, (bi.grad if with_bias else None)

    ones = torch.ones(shape, device=DEV)
    o1, gx1, gb1 = first_order(xg, ones)
    o2, gx2, gb2 = first_order(xg, None)                         # expanded scalar: stride 0
    xn = _noncontiguous(xg.detach())
    assert not xn.is_contiguous() and torch.equal(xn, xg.detach())
    o3, gx3, gb3 = first_order(xn, gog.detach())
    assert torch.equal(o1, out.detach()) and torch.equal(o2, o1) and torch.equal(o3, o1)
    assert torch.equal(gx2, gx1) and torch.equal(gx1.cpu(), _lrelu32(out_ref, ones.cpu()))
    assert torch.equal(gx3, first[0].detach())
    if with_bias:
        assert torch.equal(gb2, gb1) and torch.equal(gb3, first[1].detach())


# ---------------------------------------------------------------------------
# upfirdn2d
# ---------------------------------------------------------------------------
UFD2 = ([(shape, up, down, pad, None) for shape, up, down, pad in R.TILE_CASES]
        + [((2, 2, 13, 17), up, down, pad, kshape) for up, down, pad, kshape in R.GENERIC_CASES])


@pytest.mark.parametrize("shape,up,down,pad,kshape", UFD2)
def test_upfirdn2d_first_and_second_order(shape, up, down, pad, kshape):
    """Forward, grad_x and the gradient of (grad_x . v).sum() with respect to grad_output
    against torch autograd of upfirdn2d_native in float64 on the CPU; that second-order
    term is upfirdn2d(v): the HIP forward applied to v, bit for bit."""
    ops = R.ops
    g = torch.Generator().manual_seed(sum(shape) + up + 3 * down)
    x = torch.randn(shape, generator=g)
    k = R.blur_taps(up) if kshape is None else torch.randn(*kshape, generator=g) / 4
    v = torch.randn(shape, generator=g)
    tag = f"upfirdn2d_{'x'.join(map(str, shape))}_{up}{down}{pad}"

    x64 = x.double().requires_grad_(True)
    out_r = R.native_upfirdn2d(x64, k.double(), up=up, down=down, pad=pad)
    go = torch.randn(out_r.shape, generator=g)
    go64 = go.double().requires_grad_(True)
    gx_r, = autograd.grad(out_r, x64, go64, create_graph=True)
    ggo_r, = autograd.grad((gx_r * v.double()).sum(), go64)
    assert not R.is_zero(ggo_r)

    xg, kg = x.to(DEV).requires_grad_(True), k.to(DEV)
    gog = go.to(DEV).requires_grad_(True)
    out = ops.upfirdn2d(xg, kg, up=up, down=down, pad=pad)
    gx, = autograd.grad(out, xg, gog, create_graph=True)
    ggo, = autograd.grad((gx * v.to(DEV)).sum(), gog)
    torch.cuda.synchronize()
    _close(tag + "_fwd", out, out_r, 1e-5)
    _close(tag + "_grad_x", gx, gx_r, 1e-5)
    _close(tag + "_gradgrad_go", ggo, ggo_r, 1e-5)
    _close(tag + "_gradgrad_go_vs_native_of_v", ggo,
           R.native_upfirdn2d(v.double(), k.double(), up=up, down=down, pad=pad), 1e-5)
    with torch.no_grad():
        assert torch.equal(ggo, ops.upfirdn2d(v.to(DEV), kg, up=up, down=down, pad=pad))


# ---------------------------------------------------------------------------
# R1 and the path-length regulariser through MiniD / MiniG
# ---------------------------------------------------------------------------
def _count_kernel_calls(monkeypatch):
    """Counts the library calls the custom Functions make (the calls go through)."""
    ops = R.ops
    calls = {"fused_bias_act": 0, "fused_bias_act_mode31_bias": 0, "upfirdn2d": 0}
    fba, ufd = ops.fused_bias_act, ops._upfirdn2d_op

    def fused_bias_act(input, bias, refer, act, grad, alpha, scale):
        calls["fused_bias_act"] += 1
        calls["fused_bias_act_mode31_bias"] += grad == 1 and bias is not None and bias.numel() > 0
        return fba(input, bias, refer, act, grad, alpha, scale)

    def upfirdn2d_op(*args):
        calls["upfirdn2d"] += 1
        return ufd(*args)

    monkeypatch.setattr(ops, "fused_bias_act", fused_bias_act)
    monkeypatch.setattr(ops, "_upfirdn2d_op", upfirdn2d_op)
    return calls


def _four_ways(monkeypatch, model, inputs, run):
    """run(model, *inputs) -> {name: tensor or None} four times: the native formulas in
    float64 on the CPU (ref), in fp32 on the CPU and on the GPU (the baselines: torch ops
    only), and the HIP ops in fp32 on the GPU; with each run's leaky-ReLU record."""
    res = {}
    R.route_native(monkeypatch)
    with R.recording() as rec_ref:
        res["ref"] = run(*R.cast(model, *inputs, dtype=F64))
    res["base_cpu"] = run(*R.cast(model, *inputs))
    # cudnn off: the stacks' F.conv2d / conv_transpose2d take PyTorch's own GPU path, not
    # MIOpen, which would first have to compile kernels for these tiny channel counts
    with torch.backends.cudnn.flags(enabled=False):
        res["base_gpu"] = run(*R.cast(model, *inputs, device=DEV))
        R.route_functions(monkeypatch)
        calls = _count_kernel_calls(monkeypatch)
        with R.recording() as rec_hip:
            res["hip"] = run(*R.cast(model, *inputs, device=DEV))
        torch.cuda.synchronize()
    return res, rec_ref, rec_hip, calls


def _assert_same_branches(tag, rec_ref, rec_hip):
    """Input condition, not a tolerance: the float64 reference keeps every pre-activation
    >= 2e-5 from the kink and the HIP path's activations are within 5e-6 max(1, |ref|) of
    the reference's, so no element took the other branch (also compared directly)."""
    margin = min(r["min_abs"] for r in rec_ref)
    assert len(rec_ref) == len(rec_hip) > 0
    worst = 0.0
    for a, b in zip(rec_ref, rec_hip):
        assert a["out"].shape == b["out"].shape
        worst = max(worst, float(((b["out"] - a["out"]).abs()
                                  / a["out"].abs().clamp(min=1.0)).max()))
        assert torch.equal(a["out"] > 0, b["out"] > 0)
    _record[tag + "_kink"] = {"ref_min_abs_preactivation": margin, "activation_err": worst,
                              "leaky_relus": len(rec_ref),
                              "activations": sum(r["out"].numel() for r in rec_ref)}
    print(tag, _record[tag + "_kink"])
    assert margin >= 2e-5, margin
    assert worst <= 5e-6, worst


def _assert_parity(tag, res):
    ref = res["ref"]
    errs = {name: {way: R.rel_err(res[way][name], ref[name])
                   for way in ("hip", "base_gpu", "base_cpu")} for name in ref}
    live = [name for name in ref if not R.is_zero(ref[name])]
    bar = 4 * max(max(errs[name]["base_gpu"], errs[name]["base_cpu"]) for name in live)
    _record[tag] = {"bar": bar, "errors_over_max_ref": errs}
    print(tag, "bar %.3e" % bar)
    for name in ref:
        print(f"  {name}: " + " ".join(f"{w} {e:.3e}" for w, e in errs[name].items()))
    for name in ref:
        if name in live:
            assert errs[name]["hip"] <= bar, (name, errs[name], bar)
        else:                                   # exactly zero in float64: None or exact zeros
            assert R.is_zero(res["hip"][name]), name
    return live


# seeds by the float64 reference's kink margin alone (min |pre-activation| over all leaky
# ReLUs, searched over seeds 0..9 on the CPU): MiniD 5 -> 2.46e-4, 8 -> 1.76e-4 (4 has
# 1.07e-5: too close); MiniG 7 -> 5.02e-4, 3 -> 2.72e-4 (1 and 8 are too close)
@pytest.mark.parametrize("seed", [5, 8])
def test_r1_gradients_vs_float64(monkeypatch, seed):
    model, x = R.mini_d(seed)

    def run(m, xi):
        loss, grads = R.r1_grads(m, xi)
        return {"loss": loss, **{"grad/" + n: t for n, t in grads.items()}}

    res, rec_ref, rec_hip, calls = _four_ways(monkeypatch, model, (x,), run)
    tag = f"r1_seed{seed}"
    _record[tag + "_calls"] = calls
    # at least forward, backward and double backward of 6 leaky ReLUs and of 4 Blurs
    assert calls["fused_bias_act"] >= 18 and calls["fused_bias_act_mode31_bias"] == 6
    assert calls["upfirdn2d"] >= 12
    _assert_same_branches(tag, rec_ref, rec_hip)
    live = _assert_parity(tag, res)
    assert "loss" in live and "grad/final_linear.0.weight" in live
    assert sum(n.endswith("weight") for n in live) == 9
    for name, t in res["ref"].items():
        if name.endswith("bias"):               # piecewise linear in x
            assert R.is_zero(t), name


@pytest.mark.parametrize("seed", [7, 3])
def test_path_regularizer_gradients_vs_float64(monkeypatch, seed):
    model, *inputs = R.mini_g(seed)

    def run(m, *ins):
        penalty, lengths, grads = R.path_grads(m, *ins)
        return {"penalty": penalty, "path_lengths": lengths,
                **{"grad/" + n: t for n, t in grads.items()}}

    res, rec_ref, rec_hip, calls = _four_ways(monkeypatch, model, inputs, run)
    tag = f"path_seed{seed}"
    _record[tag + "_calls"] = calls
    # at least forward, backward and double backward of 3 leaky ReLUs, a Blur, an Upsample
    assert calls["fused_bias_act"] >= 9 and calls["fused_bias_act_mode31_bias"] == 3
    assert calls["upfirdn2d"] >= 6
    _assert_same_branches(tag, rec_ref, rec_hip)
    live = _assert_parity(tag, res)
    for name in ("penalty", "path_lengths", "grad/conv1.activate.bias", "grad/up.conv.weight",
                 "grad/up.noise.weight", "grad/to_rgb.conv.modulation.weight"):
        assert name in live, name

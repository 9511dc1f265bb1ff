"""GPU: the hash-grid table gradient on every kernel path and variant, against float64.

csrc/encoders.hip computes grad_embeddings three ways: direct atomics (B < 4096, and the
fine levels without a workspace), LDS windows (B >= 4096 without a workspace, levels of at
most 24 windows) and the binned path (a workspace, D <= 3, B >= 4096).  Every case here
restates the planning rule (tests/grid_cases.py) and asserts that it lands on the path it
is named for, then compares the HIP result with the float64 reference of tests/grid_ref.py
under the derived per-entry bound

    |got - ge| <= u ((n + 1) A + k G),   u = 2^-24,  k = D (linear) or 6 D (smoothstep)

and requires the same non-zero entries.  The assertion is the bound (ratio <= 1) and nothing
tighter; the worst err / bound per case is recorded (SDFR_PARITY_JSON, suffix
_grid_backward; the MI355X run is profiles/grid_backward_parity.json).

Cases: six (D, C, gridtype, align_corners, interpolation) variants, and a seventh with
non-integer level scales, on each path they can reach; LDS-window edges (a partial last
window, a level planned nine windows and filling four); the binned path's second sweep for
C in {8, 4, 1} with the coarse bins cut into several items; 70 000 samples at one point
(split bins on a hashed two-sweep level); the input gradient, bit for bit against the
oracle; the adjoint identity <grad, forward(E)> = <backward(grad), E> on the GPU alone; the
module path with both gradients from one backward; D = 5 forward and dy_dx bit-exact.

MI355X, worst err / bound over the cases of a path (profiles/grid_backward_parity.json):

    direct atomics (14 cases)             0.374
    LDS windows (7 cases)                 0.321     window edges (C = 8)   0.292
    binned (5 cases)                      0.313     module path            0.169
    binned second sweep, C = 8 / 4 / 1    0.407 / 0.337 / 0.342
    one point 70 000 times, g >= 0        0.0012    (one lost work item: 15.4, rejected)
    adjoint identity (7 variants)         |lhs - rhs| <= 1.5e-4 of its tolerance

The C oracle sits at the same ratios on the same inputs (test_grid_ref.py): the error
is that of the shared fp32 weights and products, not of the summation order.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import grid_cases as GC
from tests.grid_ref import assert_table_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = GC.BASE_RESOLUTION

_record = {}


def teardown_module(module):
    out = os.environ.get("SDFR_PARITY_JSON")
    if out:
        with open(out.replace(".json", "_grid_backward.json"), "w") as f:
            json.dump(_record, f, indent=1, sort_keys=True)
            f.write("\n")


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)     # a writable copy


def _forward(sdfr, d, dydx=True):
    lib = sdfr._lib
    c = d.case
    xt, et, ot = _dev(d.x), _dev(d.emb), _dev(d.offsets, np.int32)
    out = torch.empty(c.levels, c.B, c.C, device=DEV)
    dd = torch.empty(c.B, c.levels * c.D * c.C, device=DEV) if dydx else None
    lib.check(lib.lib().sdfr_grid_encode_forward(
        lib.ptr(xt), lib.ptr(et), lib.ptr(ot), lib.ptr(out), c.B, c.D, c.C, c.levels, d.S, H,
        lib.ptr(dd), c.gridtype, int(c.align), c.interp, lib.stream_of(xt)), "grid fwd")
    torch.cuda.synchronize()
    return out, dd


def _ws_bytes(sdfr, c, S):
    return sdfr._lib.lib().sdfr_grid_encode_backward_ws_bytes(c.B, c.D, c.C, c.levels, S, H,
                                                              int(c.align))


def _backward(sdfr, d, dydx=None):
    """sdfr_grid_encode_backward_ws on the case's path: with a workspace for `binned`, without
    one otherwise.  Returns (grad_embeddings, grad_inputs or None) as numpy."""
    lib = sdfr._lib
    L_ = lib.lib()
    c = d.case
    gt, xt, ot = _dev(d.g), _dev(d.x), _dev(d.offsets, np.int32)
    ge = torch.zeros(d.emb.shape, device=DEV)
    gi = torch.zeros(c.B, c.D, device=DEV) if dydx is not None else None
    wsb = _ws_bytes(sdfr, c, d.S) if c.path == "binned" else 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV) if wsb else None
    lib.check(L_.sdfr_grid_encode_backward_ws(
        lib.ptr(gt), lib.ptr(xt), None, lib.ptr(ot), lib.ptr(ge), c.B, c.D, c.C, c.levels, d.S, H,
        lib.ptr(dydx), lib.ptr(gi), c.gridtype, int(c.align), c.interp, lib.ptr(ws), wsb,
        lib.stream_of(gt)), "grid bwd ws")
    torch.cuda.synchronize()
    return ge.cpu().numpy(), (gi.cpu().numpy() if gi is not None else None)


def _assert_path(sdfr, d):
    """The case runs on the path it is named for.  `binned` asks the library
    (sdfr_grid_encode_backward_ws_bytes > 0).  `direct` and `windows` are read off the plan
    as restated in grid_cases.py, the library exposes no query for them: a change to
    kBwdLevelWins or to the window size in encoders.hip needs the same change there."""
    c = d.case
    planned = GC.planned_windows(c, d.levels)
    wsb = _ws_bytes(sdfr, c, d.S)
    if c.path == "direct":
        assert c.B < GC.MIN_BATCH and not any(planned)
    elif c.path == "windows":
        assert any(planned), planned
        if c.D > 3:
            assert wsb == 0                      # no binned path to fall onto
    else:
        assert c.path == "binned" and c.D <= 3 and wsb > 0
    return planned


@pytest.mark.parametrize("name", [c.name for c in GC.VARIANT_CASES])
def test_table_gradient_variants(sdfr, name):
    d = GC.case_data(name)
    _assert_path(sdfr, d)
    got, _ = _backward(sdfr, d)
    assert_table_grad(name, got, d.ref, _record)


def test_table_gradient_window_edges(sdfr):
    """Level 0 in one window, level 1 in two (the second partial), level 2 planned nine
    windows and filling four (`lo >= n` returns), levels 3 and 4 by direct atomics."""
    d = GC.case_data(GC.WINDOW_EDGES.name)
    assert _assert_path(sdfr, d) == [1, 2, 9, 0, 0]
    assert GC.filled_windows(d.case, d.levels)[:3] == [1, 2, 4]
    assert d.levels[1][2] % GC.window_rows(d.case.C) != 0
    got, _ = _backward(sdfr, d)
    assert_table_grad(d.case.name, got, d.ref, _record)


@pytest.mark.parametrize("name", [c.name for c in GC.SECOND_SWEEP])
def test_table_gradient_binned_second_sweep(sdfr, name):
    """A level of 64 * bin_rows<C>() rows: each of its 32 bins is two LDS windows.  The
    coarse levels' single bins hold B * 8 entries, more than one chunk: non-whole items."""
    d = GC.case_data(name)
    c = d.case
    _assert_path(sdfr, d)
    top = d.levels[-1][2]
    assert top == 64 * GC.window_rows(c.C) and GC.bin_sweeps(c, top) == 2
    # level 0 is one bin; its in-bounds entries exceed a chunk, so it is cut into items
    assert d.levels[0][2] <= GC.window_rows(c.C)
    assert d.ref.n[:int(d.offsets[1])].sum() > GC.bin_chunk(c)
    got, _ = _backward(sdfr, d)
    assert_table_grad(name, got, d.ref, _record)


def test_table_gradient_one_point_many_times(sdfr):
    """70 000 samples at one point: each touched row of the hashed two-sweep level receives
    more than a chunk, so its bin is split into non-whole items that are swept twice.  The
    gradients are all positive (ge = A): one lost item is 15 times the bound
    (test_grid_ref.py), where signed gradients would cancel and hide it."""
    d = GC.case_data(GC.ONE_POINT.name)
    c = d.case
    _assert_path(sdfr, d)
    lo = int(d.offsets[-2])
    top = d.ref.n[lo:]
    assert GC.bin_sweeps(c, d.levels[-1][2]) == 2
    assert np.count_nonzero(top) == 8 and top[top > 0].min() == c.B > GC.bin_chunk(c)
    got, _ = _backward(sdfr, d)
    assert_table_grad(c.name, got, d.ref, _record)


def _oracle_forward(oracle_mod, d):
    c = d.case
    return oracle_mod.grid_encode_forward(d.x, d.emb, d.offsets, d.pls, H, calc_dy_dx=True,
                                          gridtype=c.gridtype, align_corners=c.align,
                                          interp=c.interp)


@pytest.mark.parametrize("name", [c.name for c in GC.VARIANT_CASES if c.B in (255, 4097)])
def test_input_gradient_bit_exact(sdfr, oracle_mod, name):
    """grad_inputs is a fixed-order fma chain over dy_dx: the oracle's bits, for every
    (D, C); the forward and dy_dx that feed it are the oracle's bits too."""
    d = GC.case_data(name)
    c = d.case
    out, dd = _forward(sdfr, d)
    ref_out, ref_dd = _oracle_forward(oracle_mod, d)
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out)
    np.testing.assert_array_equal(dd.cpu().numpy(), ref_dd)
    _, gi = _backward(sdfr, d, dydx=dd)
    _, ref_gi = oracle_mod.grid_encode_backward(d.g, d.x, d.emb, d.offsets, d.pls, H,
                                                dy_dx=ref_dd, gridtype=c.gridtype,
                                                align_corners=c.align, interp=c.interp)
    assert np.abs(ref_gi).max() > 0
    np.testing.assert_array_equal(gi, ref_gi)


@pytest.mark.parametrize("C,gridtype,align,interp", [(2, 0, False, 0), (4, 1, True, 1)])
def test_grid_forward_d5_bit_exact(sdfr, oracle_mod, C, gridtype, align, interp):
    """D = 5 is accepted by the API: forward and dy_dx against the oracle, bit for bit."""
    from tests.golden import weights as W
    offsets, pls = oracle_mod.grid_offsets(num_levels=6, level_dim=C, base_resolution=8,
                                           log2_hashmap_size=15, desired_resolution=64,
                                           input_dim=5, align_corners=align)
    emb = W.det_uniform((int(offsets[-1]), C), -1, 1, 17)
    x = np.random.default_rng(50 + C).uniform(-0.02, 1.02, size=(5000, 5)).astype(np.float32)
    x[0], x[1], x[2], x[3] = 0.0, 1.0, 0.5, 0.25
    case = GC.Case("d5_forward", 5, C, gridtype, align, interp, 6, 15, len(x), "direct")
    d = SimpleNamespace(case=case, x=x, emb=emb, offsets=offsets, pls=pls,
                        S=float(np.float32(np.log2(pls))))
    out, dd = _forward(sdfr, d)
    ref_out, ref_dd = _oracle_forward(oracle_mod, d)
    assert np.count_nonzero(ref_out) > 0.7 * ref_out.size
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out)
    np.testing.assert_array_equal(dd.cpu().numpy(), ref_dd)


@pytest.mark.parametrize("name", [f"{v[0]}_{'binned' if v[1] <= 3 else 'windows'}_4097"
                                  for v in GC.VARIANTS])
def test_adjoint_identity(sdfr, name):
    """The forward is linear in the table: <grad, out> = <grad_emb, emb> in float64, with the
    HIP forward's out and the HIP backward's grad_emb.  Tolerance: the table-gradient bound
    summed against |emb| plus the forward bound summed against |grad|."""
    d = GC.case_data(name)
    out, _ = _forward(sdfr, d, dydx=False)
    ge, _ = _backward(sdfr, d)
    lhs = float((d.g.astype(np.float64) * out.cpu().numpy().astype(np.float64)).sum())
    rhs = float((ge.astype(np.float64) * d.emb.astype(np.float64)).sum())
    tol = float((d.ref.grad_bound() * np.abs(d.emb)).sum() +
                (d.ref.fwd_bound() * np.abs(d.g)).sum())
    _record["adjoint_" + name] = abs(lhs - rhs) / tol
    print(f"adjoint {name}: lhs {lhs!r} rhs {rhs!r} |diff| / tol {abs(lhs - rhs) / tol:.3e}")
    assert np.abs(d.g * out.cpu().numpy()).sum() > 1e3 * tol       # not vacuous
    assert abs(lhs - rhs) <= tol


def test_module_path_both_gradients(sdfr, oracle_mod):
    """sdfr.grid_encode with requires_grad on points and table (D = 2, C = 4, smoothstep,
    B = 4097: the module allocates the workspace, binned path): both gradients from one
    backward, the table's under the bound, the points' the oracle's bits."""
    d = GC.case_data("d2c4_smooth_binned_4097")
    c = d.case
    assert _ws_bytes(sdfr, c, d.S) > 0
    xt = _dev(d.x).requires_grad_(True)
    et = torch.nn.Parameter(_dev(d.emb))
    out = sdfr.grid_encode(xt, et, _dev(d.offsets, np.int32), d.pls, H, True, c.gridtype, c.align,
                           c.interp)
    assert out.shape == (c.B, c.levels * c.C)
    out.backward(_dev(d.g.transpose(1, 0, 2).reshape(c.B, -1)))
    assert_table_grad("module_" + c.name, et.grad.cpu().numpy(), d.ref, _record)
    _, ref_dd = _oracle_forward(oracle_mod, d)
    _, ref_gi = oracle_mod.grid_encode_backward(d.g, d.x, d.emb, d.offsets, d.pls, H,
                                                dy_dx=ref_dd, gridtype=c.gridtype,
                                                align_corners=c.align, interp=c.interp)
    np.testing.assert_array_equal(xt.grad.cpu().numpy(), ref_gi)

"""CPU: the float64 definitions and launch-arithmetic mirrors of tests/linear_ref.py, which
tests/test_gpu_linear_walk.py holds csrc/linear_f16x3.hip to -- the second-order FiLM
formulas against float64 autograd of the composite they differentiate, the walk helpers
against hand-computed cases -- and the argument checks of the sdfr_linear_* / sdfr_film_*
entry points (they reject before any launch, so no GPU is needed)."""
import itertools

import numpy as np
import pytest
import torch

from tests import linear_ref as R


def _film_inputs(F_, rows, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return dict(ds=r(F_ * rows, N), y=r(F_ * rows, N), gamma=30 + 3 * r(F_, N), beta=r(F_, N),
                g_dy=r(F_ * rows, N), g_dgamma=r(F_, N), g_dbeta=r(F_, N))


@pytest.mark.parametrize("present", list(itertools.product([True, False], repeat=3)),
                         ids=lambda p: "".join("x" if b else "-" for b in p))
def test_film_backward_grad_ref_vs_autograd(present):
    """film_backward_grad_ref == float64 autograd of du = ds cos(gamma y + beta),
    dy = du gamma, dgamma = sum du y, dbeta = sum du, for every present / absent
    combination of the three upstream gradients (absent = None = zero)."""
    F_, rows, N = 2, 5, 256
    t = _film_inputs(F_, rows, N)
    ups = [t[k] if p else None for k, p in zip(("g_dy", "g_dgamma", "g_dbeta"), present)]
    got = R.film_backward_grad_ref(t["ds"], t["y"], t["gamma"], t["beta"], *ups, rows)
    leaves = [t[k].clone().requires_grad_(True) for k in ("ds", "y", "gamma", "beta")]
    ds, y, gm, bt = leaves
    du = ds.view(F_, rows, N) * torch.cos(gm[:, None] * y.view(F_, rows, N) + bt[:, None])
    outs = [(du * gm[:, None]).reshape(-1, N), (du * y.view(F_, rows, N)).sum(1), du.sum(1)]
    # the first-order definition itself, on the way
    first = R.film_backward_ref(t["ds"], t["y"], t["gamma"], t["beta"], rows)
    for a, b in zip(first[:3], outs):
        np.testing.assert_allclose(a.numpy(), b.detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(first[3].numpy(), outs[0].detach().view(F_, rows, N).sum(1).numpy(),
                               rtol=1e-12, atol=0)
    pairs = [(o, u) for o, u in zip(outs, ups) if u is not None]
    if pairs:
        want = torch.autograd.grad([o for o, _ in pairs], leaves, [u for _, u in pairs],
                                   allow_unused=True)
        want = [torch.zeros_like(l) if w is None else w for w, l in zip(want, leaves)]
    else:
        want = [torch.zeros_like(l) for l in leaves]
    for name, a, b in zip(("d_ds", "d_y", "d_gamma", "d_beta"), got, want):
        assert a.shape == b.shape and a.dtype == torch.float64, name
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=0, err_msg=name)
    if not any(present):
        assert all(float(a.abs().max()) == 0.0 for a in got)


def test_film_ref_u32_argument():
    """With u32 the trigonometry is evaluated at exactly that argument: passing the
    float64 argument itself changes nothing, passing a shifted one shifts the cosine."""
    F_, rows, N = 2, 5, 256
    t = _film_inputs(F_, rows, N, seed=1)
    u = (t["gamma"][:, None] * t["y"].view(F_, rows, N) + t["beta"][:, None]).reshape(-1, N)
    a = R.film_backward_ref(t["ds"], t["y"], t["gamma"], t["beta"], rows)
    b = R.film_backward_ref(t["ds"], t["y"], t["gamma"], t["beta"], rows, u32=u)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    c = R.film_backward_ref(t["ds"], t["y"], t["gamma"], t["beta"], rows, u32=u + np.pi)
    np.testing.assert_allclose(c[0].numpy(), -a[0].numpy(), rtol=1e-9, atol=1e-12)
    ups = (t["g_dy"], t["g_dgamma"], t["g_dbeta"])
    a2 = R.film_backward_grad_ref(t["ds"], t["y"], t["gamma"], t["beta"], *ups, rows)
    b2 = R.film_backward_grad_ref(t["ds"], t["y"], t["gamma"], t["beta"], *ups, rows, u32=u)
    assert all(torch.equal(p, q) for p, q in zip(a2, b2))
    # the tolerance magnitudes dominate the values they bound
    for v, m in zip(a, R.film_backward_terms(t["ds"], t["y"], t["gamma"], rows)):
        assert bool((v.abs() <= m * (1 + 1e-12)).all())
    for v, m in zip(a2, R.film_backward_grad_terms(t["ds"], t["y"], t["gamma"], *ups, rows)):
        assert bool((v.abs() <= m * (1 + 1e-12)).all())


def test_wgrad_walk_hand_cases():
    assert R.wgrad_rows(4096) == 32 and R.wgrad_walk(4096) == [1] * 128
    # 40000 rows: ceil(40000 / 128) = 313 -> 320 rows = 10 m-steps, 125 workgroups
    assert R.wgrad_rows(40000) == 320 and R.wgrad_walk(40000) == [10] * 125
    # 4097 rows: 33 -> 64 rows; 65 workgroups, the last with one row
    assert R.wgrad_rows(4097) == 64 and R.wgrad_walk(4097) == [2] * 64 + [1]
    assert 4097 - 64 * 64 == 1
    # 12293 rows: 97 -> 128 rows = 4 m-steps; 97 workgroups, the last with 5 rows
    assert R.wgrad_rows(12293) == 128 and R.wgrad_walk(12293) == [4] * 96 + [1]
    assert R.wgrad_walk(1) == [1] and R.wgrad_rows(196608) == 1536
    assert R.wgrad_walk(196608) == [48] * 128


def test_fwd_walk_hand_cases():
    assert [R.fwd_nsplit(n) for n in (32, 64, 256, 272, 288)] == [1, 1, 2, 2, 2]
    # 76750 rows = 300 blocks over 128 partitions of 2 workgroups
    w = R.fwd_walk(76750, 256)
    assert len(w) == 128 and w[51] == [119, 120] and w[25] == [58, 59]
    assert w[0] == [0, 1] and w[127] == [297, 298, 299]
    assert sorted(b for ws in w for b in ws) == list(range(300))
    assert {len(ws) for ws in w} == {2, 3}
    # unsplit: 256 partitions of one workgroup walk 1 or 2 blocks
    w1 = R.fwd_walk(76750, 64)
    assert len(w1) == 256 and {len(ws) for ws in w1} == {1, 2}
    assert sorted(b for ws in w1 for b in ws) == list(range(300))
    # fewer blocks than partitions: one block each; split grids in multiples of 8
    assert R.fwd_walk(4096, 32) == [[b] for b in range(16)]
    w = R.fwd_walk(3000, 256)                      # 12 blocks -> 16 partitions
    assert len(w) == 16 and sorted(b for ws in w for b in ws) == list(range(12))
    assert max(len(ws) for ws in w) == 1
    assert R.fwd_walk(256, 256) == [[]] * 7 + [[0]]


def test_film_blocks_hand_cases():
    assert R.film_blocks(3, 701) == (11, 64) and 701 - 10 * 64 == 61
    assert R.film_blocks(1, 65) == (2, 33)
    # 171 blocks of 71 rows: block 169 holds row 11999 alone, block 170 starts past the face
    assert R.film_blocks(3, 12000) == (171, 71) and 169 * 71 == 11999 and 170 * 71 > 12000
    assert R.film_blocks(600, 64) == (1, 64)
    assert R.film_blocks(2, 98304) == (256, 384)


# ---------------------------------------------------------------------------------
# argument checks: integers stand in for pointers, nothing is dereferenced or launched
# ---------------------------------------------------------------------------------
P = [0x100000 * (i + 1) for i in range(12)]        # distinct 16-B aligned "pointers"


def _err(lib):
    return lib.sdfr_last_error()


def test_linear_argument_errors(sdfr):
    L = sdfr._lib
    lib = L.lib()
    EINVAL, EUNSUP, OK = L.SDFR_EINVAL, L.SDFR_EUNSUPPORTED, L.SDFR_OK
    # sdfr_linear_f16x3(out, x, packed, bias, M, N, K, stream)
    assert lib.sdfr_linear_f16x3(P[0], P[1], P[2], None, 4096, 256, 254, None) == EINVAL
    assert b"linear_f16x3" in _err(lib) and b"multiple of 4" in _err(lib)
    assert lib.sdfr_linear_f16x3(P[0], P[1] + 4, P[2], None, 4096, 256, 256, None) == EINVAL
    assert b"linear_f16x3" in _err(lib) and b"aligned" in _err(lib)
    assert lib.sdfr_linear_f16x3(P[0], P[1], P[2], None, 4096, 128, 256, None) == EUNSUP
    assert b"linear_f16x3" in _err(lib)
    assert lib.sdfr_linear_f16x3(None, None, None, None, 0, 256, 256, None) == OK
    # sdfr_linear_wgrad_f16x3(gw, dy, x, M, N, K, ws, ws_bytes, stream)
    need = lib.sdfr_linear_wgrad_ws_bytes(40000, 256, 256)
    assert need == 125 * 256 * 256 * 4 and lib.sdfr_linear_wgrad_ws_bytes(0, 256, 256) == 0
    assert lib.sdfr_linear_wgrad_f16x3(P[0], P[1], P[2], 40000, 128, 256, P[3], need, None) == EUNSUP
    assert b"linear_wgrad_f16x3" in _err(lib)
    assert lib.sdfr_linear_wgrad_f16x3(P[0], P[1], P[2], 40000, 256, 292, P[3], 1 << 40,
                                       None) == EUNSUP
    assert b"linear_wgrad_f16x3" in _err(lib)
    assert lib.sdfr_linear_wgrad_f16x3(P[0], P[1], P[2], 40000, 256, 256, P[3], need - 1,
                                       None) == EINVAL
    assert b"linear_wgrad_f16x3" in _err(lib) and b"workspace" in _err(lib)
    # sdfr_film_linear_f16x3(out, y_save, x, packed, bias, gamma, beta, M, N, K, rpf, stream)
    film = (P[0], P[1], P[2], P[3], None, P[4], P[5])
    assert lib.sdfr_film_linear_f16x3(*film, 4097, 256, 256, 1024, None) == EINVAL
    assert b"film_linear_f16x3" in _err(lib) and b"rows_per_face" in _err(lib)
    assert lib.sdfr_film_linear_f16x3(*film, 4096, 256, 64, 1024, None) == EUNSUP
    assert b"film_linear_f16x3" in _err(lib)
    assert lib.sdfr_film_linear_f16x3(*([None] * 7), 0, 256, 256, 1024, None) == OK
    # sdfr_film_backward(dy, dgamma, dbeta, dbf, ds, y, gamma, beta, M, N, rpf, ws, bytes, stream)
    M, rpf = 3 * 701, 701
    need = lib.sdfr_film_backward_ws_bytes(M, 256, rpf)
    assert need == 3 * 11 * 3 * 256 * 4
    assert lib.sdfr_film_backward(*P[:8], M, 256, rpf, P[8], need - 1, None) == EINVAL
    assert b"film_backward" in _err(lib) and b"workspace" in _err(lib)
    assert lib.sdfr_film_backward(*([None] * 8), 0, 256, rpf, None, 0, None) == OK
    # sdfr_film_backward_grad(d_ds, d_y, d_gamma, d_beta, ds, y, gamma, beta, g_dy, g_dgamma,
    #                         g_dbeta, M, N, rpf, ws, bytes, stream)
    need2 = lib.sdfr_film_backward_grad_ws_bytes(M, 256, rpf)
    assert need2 == need + 3 * 256 * 4
    assert lib.sdfr_film_backward_grad(*P[:8], None, None, None, M, 256, rpf, P[8], need2 - 1,
                                       None) == EINVAL
    assert b"film_backward_grad" in _err(lib) and b"workspace" in _err(lib)
    assert lib.sdfr_film_backward_grad(*([None] * 11), 0, 256, rpf, None, 0, None) == OK
    # sdfr_linear_pack(w, N, K, transposed, packed, stream)
    assert lib.sdfr_linear_pack(P[0], 0, 256, 0, P[1], None) == EINVAL
    assert b"linear_pack" in _err(lib)
    with pytest.raises(RuntimeError, match="sdfr_linear_pack"):
        L.check(EINVAL, "sdfr_linear_pack")

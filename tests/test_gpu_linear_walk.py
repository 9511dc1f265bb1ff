"""GPU: the training GEMMs and FiLM kernels (csrc/linear_f16x3.hip) each alone, through the
thin wrappers of linear.py, against float64 references of their own operation (rocBLAS
dgemm and torch elementwise ops on the device; tests/linear_ref.py) at the sizes where
their hardest code runs: several m-steps per workgroup in the weight gradient (the LDS
hand-off, the running column maxima, the consumers' rescale), several blocks per
workgroup in the persistent forward (the prefetch across a block boundary, the per-block
reset, FiLM's cached face), and the FiLM backward kernels, first and second order, element
by element.  Every coverage precondition is asserted through the launch-arithmetic mirrors
of tests/linear_ref.py (fwd_walk, wgrad_walk, film_blocks) before the kernel is called, so a
retuned kernel fails here loudly instead of losing coverage silently.

GEMM criterion (tests/test_gpu_linear.py's): per output element, |got - exact| in units of
u sum |terms| (u = 2^-24) is at most max(32, twice rocBLAS fp32's on the same data).
FiLM elementwise tolerances: derived per element from eps_t, the absolute error bound of
the device sin / cos (1e-6, measured here for cos_hw), and the fp32 roundings of each
formula; stated in the docstrings of the two FiLM backward tests.

Measured on MI355X (profiles/linear_parity.json), worst ratio per kernel:
  lin_wgrad_kernel   6.8 u ("rows", 4097 x 256; rocBLAS fp32 31.4 u); steps_up / steps_down
                     <= 1.5 u (the header's error model predicts 3-4); late_columns <= 0.54 u
  lin_fwd_kernel     14.2 u (ksteps_down, N 288 x K 256; rocBLAS fp32 22.4 u): there the
                     row maximum is set by the first k-step, each later element is off by up
                     to 2^-25 of it and the sum of terms is the first k-step's 32, so the
                     model's absolute sum allows ~13 u; ksteps_up <= 3.4 u (predicted ~3),
                     unit / rows / zero_rows <= 4.5 u; last block <= 8.1 u
  FiLM forward       y 4.5 u (rocBLAS fp32 7.0 u); out 3.8e-5 absolute, 0.064 of its bound
  cos_hw             2.5e-7 absolute over |x| <= 200
  film_bwd_kernel    dy 0.20 of its tolerance, per-face sums <= 0.039
  film_bwd2_kernel   d_ds 0.21, d_y 0.25, per-face sums <= 0.049 of their tolerances
No test failed on the committed kernels; each goes red under its mutation (the consumers'
rescale dropped, the face reload skipped, straddle blocks taken as one face, g_dgamma and
g_dbeta swapped, rows past M written).
"""
import json
import os

import pytest
import torch

from tests import linear_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
EPS_T = 1e-6          # |sin_hw - sin|, |cos_hw - cos| over |x| <= 200 (test_device_sin_accuracy)
N = 256
_record = {}


def teardown_module(module):
    out = os.environ.get("SDFR_PARITY_JSON")
    if out:
        out = out.replace(".json", "_linear.json")
        prev = {}
        if os.path.exists(out):
            with open(out) as f:
                prev = json.load(f)
        prev.update(_record)
        with open(out, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def lin(sdfr):
    from sdface_gan_amd import linear
    return linear


def _randn(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


def _rows_mag(M, seed):
    """per-row magnitudes 1e-8 .. 1e2"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return 10.0 ** (torch.rand(M, 1, generator=g, device=DEV) * 10 - 8)


def _units(got, exact, scale):
    """max |got - exact| / (u sum |terms|)"""
    return float(((got.double() - exact).abs() / (U * scale + 1e-30)).max())


def _criterion(name, got, ref32, exact, scale):
    ratio, err32 = _units(got, exact, scale), _units(ref32, exact, scale)
    _record[name] = [ratio, err32]
    print(f"{name}: {ratio:.2f} u (rocBLAS fp32 {err32:.2f} u)")
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    assert ratio <= max(32.0, 2.0 * err32), f"{name}: {ratio:.1f} u (rocBLAS {err32:.1f} u)"
    return ratio


# -----------------------------------------------------------------------------------
# weight gradient over several m-steps
# -----------------------------------------------------------------------------------
WG_SHAPES = [(4097, 256), (12293, 32), (40000, 256), (40000, 60), (40000, 272), (40000, 280),
             (40000, 4)]
WG_MAGS = ["unit", "rows", "tiny", "steps_up", "steps_down", "late_columns"]


def _wgrad_data(M, K, mag):
    gy, x = _randn((M, N), 4), _randn((M, K), 1)
    if mag == "rows":
        gy, x = gy * _rows_mag(M, 5), x * _rows_mag(M, 6)
    elif mag == "tiny":
        gy, x = gy * 1e-6, x * 1e-6
    elif mag in ("steps_up", "steps_down"):
        # rows 32 s .. 32 s + 31 (one m-step) of both operands times 4^((s % 12) - 6), or
        # 4^(6 - (s % 12)): going up, every m-step moves every column's running maximum
        # by two binades, so every step rescales the accumulators
        e = (torch.arange(M, device=DEV) // R.WGRAD_STEP_ROWS) % 12 - 6
        f = (4.0 ** (e if mag == "steps_up" else -e).float())[:, None]
        gy, x = gy * f, x * f
    elif mag == "late_columns":
        # x columns K-8 .. K-1 and gy column 17: exactly zero in the first half of every
        # workgroup's row range (their scales stay 1, then leave 1), randn after; gy
        # column 200: zero throughout
        rows = R.wgrad_rows(M)
        r = torch.arange(M, device=DEV)
        p = r // rows
        nrows = torch.clamp(M - p * rows, max=rows)
        first = (r - p * rows) < nrows // 2
        x[first, max(0, K - 8):] = 0.0
        gy[first, 17] = 0.0
        gy[:, 200] = 0.0
    return gy.contiguous(), x.contiguous()


def _wgrad_preconditions(M, mag):
    steps = R.wgrad_walk(M)
    assert max(steps) >= 2, "no workgroup runs more than one m-step"
    if M == 40000:
        assert steps == [10] * 125
    if M == 4097:
        assert steps == [2] * 64 + [1] and M - 64 * R.wgrad_rows(M) == 1
    if M == 12293:
        assert steps[0] == 4
    if mag == "steps_up":
        assert 2 <= steps[0] <= 12      # workgroup 0: the factor grows at every one of its steps
    if mag == "late_columns":
        # a full workgroup's first m-step is all zero in the late columns, a later one is not
        assert R.wgrad_rows(M) // 2 >= R.WGRAD_STEP_ROWS and steps[0] >= 2


@pytest.mark.parametrize("mag", WG_MAGS)
@pytest.mark.parametrize("M,K", WG_SHAPES)
def test_wgrad_multi_step_vs_float64(lin, M, K, mag):
    """_wgrad (lin_wgrad_kernel + lin_reduce_kernel) against gy^T x in float64 where every
    workgroup runs several m-steps of 32 rows."""
    _wgrad_preconditions(M, mag)
    gy, x = _wgrad_data(M, K, mag)
    gw = lin._wgrad(gy, x)
    gyd, xd = gy.double(), x.double()
    exact, scale = gyd.t() @ xd, gyd.abs().t() @ xd.abs()
    assert gw.shape == (N, K)
    _criterion(f"wgrad:{M}x{K}:{mag}", gw, gy.t() @ x, exact, scale)
    if mag == "late_columns":
        assert float(gw[200].abs().max()) == 0.0, "gy column 200 is zero: gw row 200 must be"
        assert float(scale[17].min()) > 0.0 and float(scale[:, K - 1].max()) > 0.0


def test_wgrad_zero_and_deterministic(lin):
    M, K = 40000, 256
    assert R.wgrad_walk(M) == [10] * 125
    gy, x = _wgrad_data(M, K, "rows")
    a, b = lin._wgrad(gy, x), lin._wgrad(gy, x)
    assert torch.equal(a, b)
    gw = lin._wgrad(torch.zeros_like(gy), x)
    assert float(gw.abs().max()) == 0.0
    gw = lin._wgrad(gy, torch.zeros_like(x))
    assert float(gw.abs().max()) == 0.0


def test_zero_rows_calls(sdfr, lin):
    """M = 0: SDFR_OK, and the weight gradient of no rows is zero."""
    L = sdfr._lib
    lib = L.lib()
    gw = torch.full((N, 64), float("nan"), device=DEV)
    st = L.stream_of(gw)
    assert lib.sdfr_linear_wgrad_f16x3(L.ptr(gw), None, None, 0, N, 64, None, 0, st) == L.SDFR_OK
    assert float(gw.abs().max()) == 0.0
    assert lib.sdfr_linear_f16x3(None, None, None, None, 0, N, 64, st) == L.SDFR_OK
    assert lib.sdfr_film_linear_f16x3(*([None] * 7), 0, N, 256, 16, st) == L.SDFR_OK
    assert lib.sdfr_film_backward(*([None] * 8), 0, N, 16, None, 0, st) == L.SDFR_OK
    assert lib.sdfr_film_backward_grad(*([None] * 11), 0, N, 16, None, 0, st) == L.SDFR_OK
    assert lib.sdfr_linear_head_forward(None, None, None, None, 0, 3, 256, st) == L.SDFR_OK


# -----------------------------------------------------------------------------------
# forward / input gradient across block boundaries
# -----------------------------------------------------------------------------------
FWD_M = 76723                      # 300 blocks of 256 rows, the last with 179
FWD_LAST = 179
# (out features, in features, transposed pack (the input gradient: B = W^T, no bias))
FWD_SHAPES = [(256, 32, False), (256, 64, False), (256, 256, False), (256, 288, False),
              (32, 256, True), (64, 256, True), (272, 256, True), (288, 256, True)]
FWD_MAGS = ["unit", "rows", "ksteps_up", "ksteps_down", "zero_rows"]


def _fwd_x(M, K, mag):
    x = _randn((M, K), 1)
    if mag == "rows":
        x = x * _rows_mag(M, 6)
    elif mag in ("ksteps_up", "ksteps_down"):
        # columns 32 q .. 32 q + 31 (one k-step) times 4^q, or 4^(KS - 1 - q): going up,
        # every row's running maximum moves two binades at every k-step, so every row
        # rescales its accumulators at every q > 0
        KS = -(-K // 32)
        q = torch.arange(K, device=DEV) // 32
        x = x * (4.0 ** (q if mag == "ksteps_up" else KS - 1 - q).float())[None, :]
    elif mag == "zero_rows":
        x[::97] = 0.0
    return x.contiguous()


def _gemm_guarded(L, x, packed, bias, n_out):
    """lin._gemm's call on an output with 256 guard rows of NaN behind it, which must
    survive: rows past M are not written."""
    M, K = x.shape
    buf = torch.full((M + 256, n_out), float("nan"), device=DEV)
    L.check(L.lib().sdfr_linear_f16x3(L.ptr(buf), L.ptr(x), L.ptr(packed), L.ptr(bias), M, n_out,
                                      K, L.stream_of(x)), "sdfr_linear_f16x3")
    assert bool(torch.isnan(buf[M:]).all()), "rows past M were written"
    return buf[:M]


def _fwd_preconditions(M, n_out):
    walk = R.fwd_walk(M, n_out)
    assert -(-M // R.FWD_BLOCK_ROWS) == 300 and M - 299 * R.FWD_BLOCK_ROWS == FWD_LAST
    assert sorted(b for w in walk for b in w) == list(range(300))
    # every workgroup walks more than one block (split kernels) / some do (unsplit)
    assert {len(w) for w in walk} == ({2, 3} if R.fwd_nsplit(n_out) == 2 else {1, 2})


@pytest.mark.parametrize("mag", FWD_MAGS)
@pytest.mark.parametrize("n_out,K,tr", FWD_SHAPES)
def test_gemm_multi_block_vs_float64(sdfr, lin, n_out, K, tr, mag):
    """_pack + sdfr_linear_f16x3 (lin_fwd_kernel) against float64 where the persistent
    workgroups walk several blocks of 256 rows; the last block's 179 rows apart."""
    M = FWD_M
    _fwd_preconditions(M, n_out)
    x = _fwd_x(M, K, mag)
    w = _randn((K, n_out) if tr else (n_out, K), 2) * 0.05
    bias = None if tr else _randn((n_out,), 3) * 0.1
    out = _gemm_guarded(sdfr._lib, x, lin._pack(w, tr), bias, n_out)
    B = w.t() if tr else w
    xd, Bd = x.double(), B.double()
    exact, scale = xd @ Bd.t(), xd.abs() @ Bd.abs().t()
    if bias is not None:
        exact, scale = exact + bias.double(), scale + bias.double().abs()
    ref32 = torch.nn.functional.linear(x, B.contiguous(), bias)
    name = f"gemm:{n_out}x{K}{'t' if tr else ''}:{mag}"
    cut = M - FWD_LAST
    _criterion(name, out[:cut], ref32[:cut], exact[:cut], scale[:cut])
    _criterion(name + ":last_block", out[cut:], ref32[cut:], exact[cut:], scale[cut:])
    if mag == "zero_rows":
        want = torch.zeros(n_out, device=DEV) if bias is None else bias
        assert torch.equal(out[::97], want.expand(out[::97].shape))


def test_gemm_wrapper_is_the_guarded_call(sdfr, lin):
    """lin._gemm returns what the guarded call of the test above returns, bit for bit."""
    x, w = _fwd_x(FWD_M, 256, "rows"), _randn((N, 256), 2) * 0.05
    bias = _randn((N,), 3) * 0.1
    packed = lin._pack(w, False)
    assert torch.equal(lin._gemm(x, packed, bias, N), _gemm_guarded(sdfr._lib, x, packed, bias, N))


# -----------------------------------------------------------------------------------
# FiLM forward: the face cache
# -----------------------------------------------------------------------------------
def _block_faces(M, rows_per_face):
    """(face of the first row, face of the last row) per block of 256 rows (:232)."""
    nblk = -(-M // R.FWD_BLOCK_ROWS)
    return [((b * 256) // rows_per_face, (min(M, (b + 1) * 256) - 1) // rows_per_face)
            for b in range(nblk)]


def _film_fwd_preconditions(F_, rpf):
    M = F_ * rpf
    walk, faces = R.fwd_walk(M, N), _block_faces(M, rpf)
    straddle = [b for b, (f0, f1) in enumerate(faces) if f0 != f1]
    if rpf == 15350:
        assert straddle == [59, 119, 179, 239]
        # a cached face, then a straddle block; a straddle block first, then another face
        assert walk[25] == [58, 59] and faces[58] == (0, 0)
        assert walk[51] == [119, 120] and faces[119] == (1, 2) and faces[120] == (2, 2)
    else:
        assert rpf == 15360 and straddle == []
        assert walk[25] == [58, 59] and faces[58] == faces[59] == (0, 0)       # reuse
        assert walk[51] == [119, 120] and faces[119] == (1, 1) and faces[120] == (2, 2)  # reload
    assert all(len(w) >= 2 for w in walk)


@pytest.mark.parametrize("rpf,K", [(15350, 256), (15360, 256), (15350, 272)])
def test_film_forward_face_cache_vs_float64(lin, rpf, K):
    """_film_fwd (lin_fwd_kernel<.., FILM>): y against float64 by the GEMM criterion, out by
    test_film_linear_vs_float64's argument-scaled bound, where workgroups keep, reload and
    bypass (straddle blocks) their cached face's gamma / beta.  Per-face offsets on gamma
    and beta make a stale or wrong face miss by O(1)."""
    F_ = 5
    M = F_ * rpf
    _film_fwd_preconditions(F_, rpf)
    x = _randn((M, K), 5) * 0.5
    w, b = _randn((N, K), 6) * 0.05, _randn((N,), 7) * 0.1
    f = torch.arange(F_, device=DEV, dtype=torch.float32)[:, None]
    gam = 30 + 3 * _randn((F_, N), 8) + 2 * f
    bet = 0.25 * _randn((F_, N), 9) + 5 * f
    out, y = lin._film_fwd(x, lin._pack(w, False), b, gam, bet, N)
    xd, wd, bd = x.double(), w.double(), b.double()
    yd, yscale = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
    name = f"film_fwd:{F_}x{rpf}x{K}"
    _criterion(name + ":y", y, torch.nn.functional.linear(x, w, b), yd, yscale)
    gd, btd = (t.double().repeat_interleave(rpf, 0) for t in (gam, bet))
    sd = torch.sin(gd * yd + btd)
    arg_err = 64 * U * (gd.abs() * yscale + btd.abs()) + 1.5e-6
    err = (out.double() - sd).abs()
    _record[name + ":out"] = [float(err.max()), float((err / arg_err).max())]
    print(f"{name}:out: max err {float(err.max()):.3e}, {float((err / arg_err).max()):.3f} of bound")
    assert float((err - arg_err).max()) <= 0
    # the straddle blocks' rows by themselves, so a failure there is named
    for blk, (f0, f1) in enumerate(_block_faces(M, rpf)):
        if f0 != f1:
            s = slice(blk * 256, (blk + 1) * 256)
            assert float((err[s] - arg_err[s]).max()) <= 0, f"straddle block {blk}"


# -----------------------------------------------------------------------------------
# FiLM backward, first and second order, elementwise
# -----------------------------------------------------------------------------------
def test_device_cos_accuracy(lin):
    """cos_hw (the FiLM backward kernels' cosine: fma 2 pi reduction + v_cos_f32) through
    film_bwd_kernel with ds = gamma = 1, beta = 0, so dy = cos_hw(y): within the 1e-6 that
    test_device_sin_accuracy asserts for its twin sin_hw, over the same range."""
    rows = 4096
    g = torch.Generator(device=DEV).manual_seed(0)
    y = ((torch.rand(rows, N, generator=g, device=DEV, dtype=torch.float64) - 0.5) * 400).float()
    one, zero = torch.ones(1, N, device=DEV), torch.zeros(1, N, device=DEV)
    dy, _, _, _ = lin._film_bwd(torch.ones_like(y), y, one, zero)
    err = float((dy.double() - torch.cos(y.double())).abs().max())
    _record["cos_hw:max_abs_err"] = err
    _record["eps_t"] = EPS_T
    print(f"cos_hw: max abs err {err:.3e}")
    assert err < 1e-6
    assert err <= EPS_T


FILM_SHAPES = [(3, 701), (1, 65), (3, 12000), (600, 64)]


def _film_data(F_, rows):
    M = F_ * rows
    f = torch.arange(F_, device=DEV, dtype=torch.float32)[:, None]
    t = dict(ds=_randn((M, N), 10), y=_randn((M, N), 11) * 0.7,          # |y| up to ~3
             gamma=30 + 3 * _randn((F_, N), 8),                            # 30 +- 9
             beta=0.25 * _randn((F_, N), 9) + 0.5 * (f % 7),
             g_dy=_randn((M, N), 12), g_dgamma=_randn((F_, N), 13), g_dbeta=_randn((F_, N), 14))
    # the sin / cos argument as the kernels form it: fl(fl(gamma y) + beta), two fp32 ops
    prod = t["gamma"][:, None] * t["y"].view(F_, rows, N)
    t["u32"] = (prod + t["beta"][:, None]).reshape(M, N)
    return t


def _film_preconditions(F_, rows):
    nb, rpb = R.film_blocks(F_, rows)
    if (F_, rows) == (3, 701):        # the 4-row unrolled loop and its tail
        assert (nb, rpb) == (11, 64) and rows - 10 * rpb == 61 and 61 % 4 != 0
    elif (F_, rows) == (1, 65):
        assert (nb, rpb) == (2, 33) and rows - rpb == 32
    elif (F_, rows) == (3, 12000):    # an empty trailing block behind a one-row block
        assert (nb - 1) * rpb >= rows and (nb - 2) * rpb == rows - 1
    else:
        assert nb == 1 and F_ > 512
    # the longest chain of fp32 additions behind one per-face sum: a block's rows
    # (film_bwd_kernel, one thread per column), ceil(nb / 8) block partials per group and
    # the 8 group sums (film_bwd_reduce_kernel)
    return rpb + -(-nb // 8) + 8


def _tol_check(name, got, ref, tol):
    err = (got.double() - ref).abs()
    ratio = float((err / (tol + 1e-300)).max())
    _record[name] = ratio
    print(f"{name}: {ratio:.3f} of tolerance")
    assert bool(torch.isfinite(got).all()), name
    assert ratio <= 1.0, f"{name}: max err / tolerance = {ratio:.3f}"


@pytest.mark.parametrize("F_,rows", FILM_SHAPES)
def test_film_backward_elementwise(lin, F_, rows):
    """_film_bwd (film_bwd_kernel + film_bwd_reduce_kernel) against linear_ref.
    Tolerances: dy = fl(fl(ds cos_hw(u)) gamma), three roundings and eps_t on the cosine:
    |ds gamma| (eps_t + 8 u); a per-face sum over a chain of n fp32 additions:
    (eps_t + n u) sum |terms|, the terms with |cos| = 1."""
    n = _film_preconditions(F_, rows)
    t = _film_data(F_, rows)
    args = (t["ds"], t["y"], t["gamma"], t["beta"])
    got = lin._film_bwd(*args)
    ref = R.film_backward_ref(*args, rows, u32=t["u32"])
    mag = R.film_backward_terms(t["ds"], t["y"], t["gamma"], rows)
    name = f"film_bwd:{F_}x{rows}"
    _tol_check(name + ":dy", got[0], ref[0], mag[0] * (EPS_T + 8 * U))
    for k, g, r, m in zip(("dgamma", "dbeta", "dbf"), got[1:], ref[1:], mag[1:]):
        assert g.shape == (F_, N)
        _tol_check(f"{name}:{k}", g, r, m * (EPS_T + n * U))
    again = lin._film_bwd(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


_ALL8 = [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)]
FILM2_CASES = ([(3, 701, p) for p in _ALL8] +
               [(F_, rows, p) for F_, rows in FILM_SHAPES[1:]
                for p in ((True, True, True), (True, False, False))])


@pytest.mark.parametrize("F_,rows,present", FILM2_CASES,
                         ids=lambda v: "".join("x" if b else "-" for b in v)
                         if isinstance(v, tuple) else str(v))
def test_film_backward_grad_elementwise(lin, F_, rows, present):
    """_film_bwd2 (film_bwd2_kernel + film_bwd_reduce_kernel) against linear_ref for every
    present / absent combination of the upstream gradients.  With A = |g_dy gamma| +
    |g_dgamma y| + |g_dbeta| (H in fp32: two additions), eps_t on cos and sin:
    d_ds: A (eps_t + 8 u);  d_y: (A |ds gamma| + |g_dgamma ds|) (eps_t + 8 u);
    per-face sums: (eps_t + n u) sum |terms|.  All absent: exact zeros."""
    n = _film_preconditions(F_, rows)
    t = _film_data(F_, rows)
    ups = [t[k] if p else None for k, p in zip(("g_dy", "g_dgamma", "g_dbeta"), present)]
    args = (t["ds"], t["y"], t["gamma"], t["beta"], *ups)
    got = lin._film_bwd2(*args)
    ref = R.film_backward_grad_ref(*args, rows, u32=t["u32"])
    mag = R.film_backward_grad_terms(t["ds"], t["y"], t["gamma"], *ups, rows)
    name = f"film_bwd2:{F_}x{rows}:" + "".join("x" if p else "-" for p in present)
    _tol_check(name + ":d_ds", got[0], ref[0], mag[0] * (EPS_T + 8 * U))
    _tol_check(name + ":d_y", got[1], ref[1], mag[1] * (EPS_T + 8 * U))
    _tol_check(name + ":d_gamma", got[2], ref[2], mag[2] * (EPS_T + n * U))
    _tol_check(name + ":d_beta", got[3], ref[3], mag[3] * (EPS_T + n * U))
    if not any(present):
        assert all(float(g.abs().max()) == 0.0 for g in got)
    else:
        assert all(float(r.abs().max()) > 0.0 for r in ref)
    again = lin._film_bwd2(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))

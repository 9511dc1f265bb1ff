"""Float64 torch definitions of the FiLM backward's elementwise part, first and second
order (include/sdfr.h, "Renderer MLP linear layers for training"), and pure-Python mirrors
of the training GEMMs' launch arithmetic: what csrc/linear_f16x3.hip is held to and how the
GPU tests prove which of its paths their shapes reach.  Test infrastructure; the product
never falls back to it.  Device-agnostic: every result lives where its inputs live.

  film_backward_ref(ds, y, gamma, beta, R, u32=None)
        dy [M,N], dgamma, dbeta, dbf [F,N] of sdfr_film_backward
  film_backward_grad_ref(ds, y, gamma, beta, g_dy, g_dgamma, g_dbeta, R, u32=None)
        d_ds, d_y [M,N], d_gamma, d_beta [F,N] of sdfr_film_backward_grad (None = zero)
  film_backward_terms / film_backward_grad_terms
        the magnitudes the tests' tolerances are stated in (every |cos|, |sin| taken as 1)
  fwd_walk(M, N)        blocks of 256 rows each row partition of lin_fwd_kernel walks
  fwd_nsplit(N)         workgroups (output-tile splits) per row partition
  wgrad_rows(M), wgrad_walk(M)
                        rows per workgroup of lin_wgrad_kernel; m-steps per workgroup
  film_blocks(F, R)     (blocks per face, rows per block) of film_bwd / film_bwd2_kernel

ds, y are [M, N] with M = F R (F faces of R consecutive rows); gamma, beta [F, N].
``u32``: the sin / cos argument as the kernels form it, fp32 fl(fl(gamma y) + beta); when
given the trigonometry is evaluated in float64 at exactly that argument, so a comparison
excludes the argument's own rounding (|u| ~ 100: ~1e-5), which the fp32 formulation of
the operation shares with the reference's separate elementwise ops.
"""
import torch


def _faces(t, R):
    t = t.double()
    return t.view(-1, R, t.shape[-1])                   # [F, R, N]


def _args(ds, y, gamma, beta, R, u32):
    dsf, yf = _faces(ds, R), _faces(y, R)
    gm, bt = gamma.double()[:, None], beta.double()[:, None]     # [F, 1, N]
    u = gm * yf + bt if u32 is None else _faces(u32, R)
    return dsf, yf, gm, bt, u


def film_backward_ref(ds, y, gamma, beta, R, u32=None):
    """du = ds cos(u), u = gamma[f] y + beta[f]: dy = du gamma[f]; per face
    dgamma = sum du y, dbeta = sum du, dbf = sum dy (include/sdfr.h:669-672)."""
    N = y.shape[-1]
    dsf, yf, gm, _, u = _args(ds, y, gamma, beta, R, u32)
    du = dsf * torch.cos(u)
    dy = du * gm
    return dy.reshape(-1, N), (du * yf).sum(1), du.sum(1), dy.sum(1)


def film_backward_terms(ds, y, gamma, R):
    """Magnitudes of film_backward_ref's outputs with |cos| = 1: |ds gamma| [M,N] and the
    per-face sums of |ds y|, |ds|, |ds gamma| [F,N]."""
    N = y.shape[-1]
    dsf, yf = _faces(ds, R).abs(), _faces(y, R).abs()
    gm = gamma.double()[:, None].abs()
    return (dsf * gm).reshape(-1, N), (dsf * yf).sum(1), dsf.sum(1), (dsf * gm).sum(1)


def _upstream(g_dy, g_dgamma, g_dbeta, yf, gm, R):
    gd = torch.zeros_like(yf) if g_dy is None else _faces(g_dy, R)
    gg = torch.zeros_like(gm) if g_dgamma is None else g_dgamma.double()[:, None]
    gb = torch.zeros_like(gm) if g_dbeta is None else g_dbeta.double()[:, None]
    return gd, gg, gb


def film_backward_grad_ref(ds, y, gamma, beta, g_dy, g_dgamma, g_dbeta, R, u32=None):
    """include/sdfr.h:682-690.  With H = g_dy gamma[f] + g_dgamma[f] y + g_dbeta[f]:
    d_ds = H cos u;  d_y = -H ds sin u gamma[f] + g_dgamma[f] ds cos u;
    d_gamma[f] = sum (-H ds sin u y + g_dy ds cos u);  d_beta[f] = sum -H ds sin u."""
    N = y.shape[-1]
    dsf, yf, gm, _, u = _args(ds, y, gamma, beta, R, u32)
    gd, gg, gb = _upstream(g_dy, g_dgamma, g_dbeta, yf, gm, R)
    cu, su = torch.cos(u), torch.sin(u)
    H = gd * gm + gg * yf + gb
    dU = -H * dsf * su
    d_ds = H * cu
    d_y = dU * gm + gg * dsf * cu
    return (d_ds.reshape(-1, N), d_y.reshape(-1, N), (dU * yf + gd * dsf * cu).sum(1), dU.sum(1))


def film_backward_grad_terms(ds, y, gamma, g_dy, g_dgamma, g_dbeta, R):
    """Magnitudes of film_backward_grad_ref's outputs with |cos| = |sin| = 1 and
    A = |g_dy gamma| + |g_dgamma y| + |g_dbeta|:  A,  A |ds gamma| + |g_dgamma ds|  [M,N];
    per-face sums of  A |ds y| + |g_dy ds|  and  A |ds|  [F,N]."""
    N = y.shape[-1]
    dsf, yf = _faces(ds, R).abs(), _faces(y, R).abs()
    gm = gamma.double()[:, None].abs()
    gd, gg, gb = (t.abs() for t in _upstream(g_dy, g_dgamma, g_dbeta, yf, gm, R))
    A = gd * gm + gg * yf + gb
    return (A.reshape(-1, N), (A * dsf * gm + gg * dsf).reshape(-1, N),
            (A * dsf * yf + gd * dsf).sum(1), (A * dsf).sum(1))


# ---------------------------------------------------------------------------------
# launch arithmetic of csrc/linear_f16x3.hip, mirrored (line numbers of that file)
# ---------------------------------------------------------------------------------
FWD_BLOCK_ROWS = 256        # kLinRows, :54: rows of x per forward block
FWD_WORKGROUPS = 256        # launch_fwd, :743: G = 256 / NSPLIT row partitions
WGRAD_STEP_ROWS = 32        # lin_wgrad_kernel, :558: nsteps = ceil(nrows / 32)
WGRAD_RANGES = 128          # wgrad_rows, :732: 128 row ranges
FILM_BLOCKS = 512           # film_blocks_per_face, :751: ~512 blocks in all
FILM_MIN_ROWS = 64          # film_blocks_per_face, :752: at least 64 rows each


def _cdiv(a, b):
    return -(-a // b)


def fwd_nsplit(N):
    """fwd_ntw / fwd_nsplit, :138-141: more than 9 output tiles of 16 are split in two."""
    NT = _cdiv(N, 16)
    ntw = (NT + 1) // 2 if NT > 9 else NT
    return _cdiv(NT, ntw)


def fwd_walk(M, N):
    """The blocks (of 256 rows) row partition w = 0..G-1 of lin_fwd_kernel walks, in order:
    [b0, b1) with b0 = w nblk / G (:175-177); G as launch_fwd chooses it (:741-744).  Each
    partition is fwd_nsplit(N) workgroups walking the same blocks."""
    ns = fwd_nsplit(N)
    nblk = _cdiv(M, FWD_BLOCK_ROWS)
    G = FWD_WORKGROUPS // ns
    if nblk < G:
        G = max(8, _cdiv(nblk, 8) * 8) if ns > 1 else nblk
    return [list(range(w * nblk // G, (w + 1) * nblk // G)) for w in range(G)]


def wgrad_rows(M):
    """wgrad_rows, :730-734: rows per workgroup, whole m-steps."""
    return max(WGRAD_STEP_ROWS,
               _cdiv(_cdiv(M, WGRAD_RANGES), WGRAD_STEP_ROWS) * WGRAD_STEP_ROWS)


def wgrad_walk(M):
    """m-steps of workgroup p = 0..P-1 of lin_wgrad_kernel (P = ceil(M / rows), :948;
    nrows = min(rows, M - p rows), nsteps = ceil(nrows / 32), :556-558)."""
    rows = wgrad_rows(M)
    return [_cdiv(min(rows, M - p * rows), WGRAD_STEP_ROWS) for p in range(_cdiv(M, rows))]


def film_blocks(F, R):
    """(nb, rpb) of sdfr_film_backward / _grad: film_blocks_per_face, :749-754, and
    rpb = ceil(R / nb), :843.  Block j of a face covers its rows [j rpb, min(R, (j+1) rpb))."""
    nb = max(1, min(_cdiv(FILM_BLOCKS, F), _cdiv(R, FILM_MIN_ROWS)))
    return nb, _cdiv(R, nb)

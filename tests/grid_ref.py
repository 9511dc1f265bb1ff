"""A float64 statement of the hash-grid table gradient, and the comparison it allows.

The reference is written from the math, not from an implementation.  For every
in-bounds (sample, level, corner) it forms

* the table row, in exact integer arithmetic: the dense index sum(p_d * s^d) over the
  dimensions whose stride s^d does not exceed the level's hashmap size (s = res + 1, or
  res with align_corners), replaced by the XOR of p_d * prime_d mod 2^32 when the grid
  is hashed and the full stride exceeds the hashmap size, then ``% hashmap_size``;
* the weight, in float64: p = x * scale + (0 or 0.5) formed in float64 and rounded once
  to float32 (the one rounding every implementation shares, because floor(p) decides the
  cell), floor(p) and p - floor(p) exact, smoothstep and the (1 - f) / f products in
  float64.

Only the per-level (scale, resolution, hashmap_size) come from ``oracle.level_table``.

Per table entry, accumulated with ``np.add.at`` in float64:

    ge  sum of w * g           the gradient
    A   sum of |w * g|
    G   sum of |g|
    n   contributions (per row)

and per (level, sample, channel) the forward value sum of w * v, V = sum of |w * v| and
vmax = max |v| over the corners.

The comparison.  An fp32 implementation forms each product fl(w) * g in fp32 and sums n
of them in some order.  With u = 2^-24, for any order,

    |got - ge| <= u * ((n + 1) * A + k * G),      k = D (linear), 6 * D (smoothstep)

(one rounding per product and n - 1 roundings of partial sums bounded by A; plus the
absolute error of an fp32 weight, D factors <= 1 with one rounding each when linear and
at most six with smoothstep, times |g|).  ``assert_table_grad`` applies it entrywise with
no free constant, and asserts that ``got`` and ``ge`` are non-zero in the same entries.
One exemption is forced by fp32 itself: smoothstep(f) rounds to 1 for 1 - f < ~1e-4, so
the fp32 weight (1 - s) is exactly 0 where the float64 one is ~1e-9.  ``sure`` counts,
per entry, the contributions with g != 0 whose fp32 weight cannot be zero: with
smoothstep, every weight factor exceeds its fp32 error (six roundings of u); with linear
weights, every factor is non-zero (f is exact in fp32), so the exemption never applies
to a linear case.  An entry with ge != 0 may be zero in ``got`` only if it has no such
contribution.  An entry with ge == 0 must be exactly zero.
The forward's bound per output is u * ((2^D + 1) * V + k * vmax).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737)


@dataclass
class GridRef:
    ge: np.ndarray          # [rows, C] float64
    A: np.ndarray           # [rows, C]
    G: np.ndarray           # [rows, C]
    n: np.ndarray           # [rows] int64
    sure: np.ndarray        # [rows, C] contributions that no fp32 rounding can make zero
    fwd: np.ndarray         # [L, B, C] float64
    V: np.ndarray           # [L, B, C]
    vmax: np.ndarray        # [L, B, C]
    k: int                  # D (linear) or 6 * D (smoothstep)
    D: int
    offsets: np.ndarray     # [L + 1]
    entries: list           # per level: (sample [E], global row [E], weight [E])

    def grad_bound(self):
        return U * ((self.n[:, None] + 1.0) * self.A + self.k * self.G)

    def fwd_bound(self):
        return U * ((2 ** self.D + 1.0) * self.V + self.k * self.vmax)

    def level_of(self, row):
        return int(np.searchsorted(self.offsets, row, side="right") - 1)


def level_rows(pl, res, hsize, gridtype, align_corners):
    """Table row of integer grid points ``pl`` [E, D] (int64) on one level."""
    D = pl.shape[1]
    s = res if align_corners else res + 1
    stride, ndims = 1, 0
    while ndims < D and stride <= hsize:
        stride *= s
        ndims += 1
    if gridtype == 0 and stride > hsize:
        index = np.zeros(pl.shape[0], np.int64)
        for d in range(D):
            index ^= (pl[:, d] * PRIMES[d]) % (1 << 32)      # < 2^9 * 2^32: exact in int64
    else:
        index = np.zeros(pl.shape[0], np.int64)
        for d in range(ndims):
            index += pl[:, d] * (s ** d)
    return index % hsize


def level_fractions(x, scale, align_corners, interp):
    """Cell [B, D] (int64) and in-cell weight f [B, D] (float64) of float32 points x."""
    p = (x.astype(np.float64) * np.float64(scale) + (0.0 if align_corners else 0.5))
    p = p.astype(np.float32).astype(np.float64)              # the one shared rounding
    cell = np.floor(p)
    f = p - cell                                             # exact
    if interp == 1:
        f = f * f * (3.0 - 2.0 * f)
    return cell.astype(np.int64), f


def grid_reference(grad, x, emb, offsets, levels, gridtype=0, align_corners=False, interp=0,
                   frac_hook=None):
    """grad [L, B, C], x [B, D] float32, emb [rows, C], ``levels`` = oracle.level_table(...).
    ``frac_hook(level, f) -> f`` lets a test damage the weights of a level."""
    x = np.asarray(x, np.float32)
    g64 = np.asarray(grad, np.float64)
    e64 = np.asarray(emb, np.float64)
    offsets = np.asarray(offsets, np.int64)
    L, B, C = g64.shape
    D = x.shape[1]
    rows_total = e64.shape[0]
    ge = np.zeros((rows_total, C))
    A = np.zeros((rows_total, C))
    G = np.zeros((rows_total, C))
    n = np.zeros(rows_total, np.int64)
    sure = np.zeros((rows_total, C), np.int64)
    k = 6 * D if interp == 1 else D
    fwd = np.zeros((L, B, C))
    V = np.zeros((L, B, C))
    vmax = np.zeros((L, B, C))
    entries = []
    inb = np.flatnonzero(np.all((x >= 0) & (x <= 1), axis=1))
    bits = (np.arange(1 << D)[:, None] >> np.arange(D)[None, :]) & 1          # [2^D, D]
    for l, (scale, res, hsize) in enumerate(levels):
        cell, f = level_fractions(x[inb], scale, align_corners, interp)
        if frac_hook is not None:
            f = frac_hook(l, f)
        w = np.ones((len(inb), 1 << D))
        fmin = np.ones((len(inb), 1 << D))
        for d in range(D):
            fac = np.where(bits[None, :, d] == 1, f[:, d:d + 1], 1.0 - f[:, d:d + 1])
            w *= fac
            fmin = np.minimum(fmin, fac)
        pl = (cell[:, None, :] + bits[None, :, :]).reshape(-1, D)
        row = int(offsets[l]) + level_rows(pl, int(res), int(hsize), gridtype, align_corners)
        samp = np.repeat(inb, 1 << D)
        wf = w.reshape(-1)
        gl = g64[l][samp]                                                      # [E, C]
        wg = wf[:, None] * gl
        np.add.at(ge, row, wg)
        np.add.at(A, row, np.abs(wg))
        np.add.at(G, row, np.abs(gl))
        np.add.at(n, row, 1)
        # the fp32 weight cannot be zero: smoothstep, every factor above its fp32 error (six
        # roundings); linear, every factor non-zero (f is exact in fp32 and 1 - f rounds to
        # zero only when f is exactly 1)
        floor = 6 * U if interp == 1 else 0.0
        np.add.at(sure, row, (fmin.reshape(-1, 1) > floor) & (gl != 0))
        v = e64[row]                                                           # [E, C]
        wv = (wf[:, None] * v).reshape(len(inb), 1 << D, C)
        fwd[l, inb] = wv.sum(1)
        V[l, inb] = np.abs(wv).sum(1)
        vmax[l, inb] = np.abs(v).reshape(len(inb), 1 << D, C).max(1)
        entries.append((samp, row, wf))
    return GridRef(ge, A, G, n, sure, fwd, V, vmax, k, D, offsets, entries)


def assert_table_grad(name, got, ref, record=None):
    """Entrywise |got - ge| <= u ((n + 1) A + k G), same non-zero entries.  Returns the worst
    err / bound and stores it in ``record[name]``."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.ge.shape, (got.shape, ref.ge.shape)
    err = np.abs(got - ref.ge)
    bound = ref.grad_bound()
    live = bound > 0
    ratio = np.zeros_like(err)
    ratio[live] = err[live] / bound[live]
    worst = float(ratio.max()) if ratio.size else 0.0
    if record is not None:
        record[name] = worst
    print(f"{name}: worst err / bound {worst:.3f}")

    def where(mask):
        r, c = np.argwhere(mask)[0]
        lv = ref.level_of(r)
        return (f"level {lv} row {r - int(ref.offsets[lv])} channel {c}: got {got[r, c]!r} "
                f"ref {ref.ge[r, c]!r} n {int(ref.n[r])} A {ref.A[r, c]:.3e} bound "
                f"{bound[r, c]:.3e}")

    # non-zero in the same entries.  The one exemption: an entry all of whose contributions
    # have a weight factor within the fp32 weight error of zero (smoothstep(f) rounding to 1
    # makes 1 - s exactly 0 in fp32) may be zero in ``got``.
    pattern = ((got != 0) & (ref.ge == 0)) | ((got == 0) & (ref.sure > 0))
    assert not pattern.any(), (f"{name}: {int(pattern.sum())} entries non-zero on one side only; "
                               + where(pattern))
    dead = ~live & (err > 0)
    assert not dead.any(), f"{name}: non-zero where nothing contributes; " + where(dead)
    bad = err > bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} entries over the bound, worst ratio "
                           f"{worst:.3f}; " + where(ratio == ratio.max()))
    return worst


def assert_forward(name, got, ref):
    """Entrywise |got - fwd| <= u ((2^D + 1) V + k vmax).  Returns the worst err / bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.fwd.shape, (got.shape, ref.fwd.shape)
    err = np.abs(got - ref.fwd)
    bound = ref.fwd_bound()
    live = bound > 0
    assert not (err[~live] > 0).any(), f"{name}: non-zero output where no row contributes"
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print(f"{name}: forward worst err / bound {worst:.3f}")
    assert worst <= 1.0, f"{name}: forward err / bound {worst:.3f}"
    return worst

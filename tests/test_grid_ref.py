"""The float64 hash-grid reference (tests/grid_ref.py) against the C oracle, on exactly the
inputs test_gpu_grid_backward.py uses: the p rounding and the index math agree (same
non-zero entries, every entry inside the derived bound), the forward agrees, and the
comparison rejects a table gradient with one contribution dropped, doubled or moved (in the
one-point case, where no row is sparse: one lost work item), one level's weights mirrored on
an axis, or linear weights where smoothstep was asked for."""
import numpy as np
import pytest

from tests import grid_cases as GC
from tests.grid_ref import assert_forward, assert_table_grad, grid_reference

NAMES = [c.name for c in GC.ALL_CASES]


def _oracle_grad(oracle_mod, d):
    c = d.case
    ge, _ = oracle_mod.grid_encode_backward(d.g, d.x, d.emb, d.offsets, d.pls, GC.BASE_RESOLUTION,
                                            gridtype=c.gridtype, align_corners=c.align,
                                            interp=c.interp)
    return ge


@pytest.fixture(scope="module", params=NAMES)
def name(request):
    """Module-scoped, so that pytest runs the tests of one case next to each other and
    grid_cases.case_data computes each reference once."""
    return request.param


def test_reference_gradient_vs_oracle(oracle_mod, name):
    d = GC.case_data(name)
    assert_table_grad(name, _oracle_grad(oracle_mod, d), d.ref)
    for l in range(d.case.levels):                                   # every level contributes
        assert d.ref.n[d.offsets[l]:d.offsets[l + 1]].sum() > 0


def test_reference_forward_vs_oracle(oracle_mod, name):
    d = GC.case_data(name)
    c = d.case
    out, _ = oracle_mod.grid_encode_forward(d.x, d.emb, d.offsets, d.pls, GC.BASE_RESOLUTION,
                                            gridtype=c.gridtype, align_corners=c.align,
                                            interp=c.interp)
    assert_forward(name, out, d.ref)


def _sparse_contribution(d):
    """(row, sample, level, weight): the heaviest contribution to the first table row, from
    the finest level down, that receives at most 8 and has a neighbour row in its level."""
    ref = d.ref
    for l in reversed(range(d.case.levels)):
        lo, hi = int(d.offsets[l]), int(d.offsets[l + 1])
        samp, row, w = ref.entries[l]
        cand = np.flatnonzero((ref.n[lo:hi - 1] > 0) & (ref.n[lo:hi - 1] <= 8)) + lo
        for r in cand:
            e = np.flatnonzero(row == r)
            k = e[np.argmax(np.abs(w[e]))]
            if w[k] >= 0.05:
                return int(r), int(samp[k]), l, float(w[k])
    raise AssertionError("no table row with at most 8 contributions: use fewer samples per row")


def _rejected(name, table, ref):
    with pytest.raises(AssertionError):
        assert_table_grad(name, table, ref)


def test_comparison_rejects_damaged_tables(oracle_mod, name):
    d = GC.case_data(name)
    c = d.case
    good = _oracle_grad(oracle_mod, d)
    if c.one_point:
        # every touched row receives all 70 000 samples, there is no sparse row: the damage
        # is one lost work item instead.  The binned path cuts a top-level row's 70 000
        # entries into items of bin_chunk and the rest; drop the smaller one from one row.
        top = c.levels - 1
        samp, row, w = d.ref.entries[top]
        r = int(row[0])
        lost = np.flatnonzero(row == r)[GC.bin_chunk(c):]
        assert 0 < len(lost) < GC.bin_chunk(c)
        item = (w[lost, None] * d.g[top][samp[lost]].astype(np.float64)).sum(0)
        damaged = good.copy()
        damaged[r] = (good[r].astype(np.float64) - item).astype(np.float32)
        _rejected(name + " lost item", damaged, d.ref)
    else:
        r, b, l, w = _sparse_contribution(d)
        contrib = (np.float32(w) * d.g[l, b]).astype(np.float32)
        dropped = good.copy()
        dropped[r] -= contrib                                        # (a)
        _rejected(name + " dropped", dropped, d.ref)
        doubled = good.copy()
        doubled[r] += contrib                                        # (b)
        _rejected(name + " doubled", doubled, d.ref)
        moved = dropped.copy()
        moved[r + 1] += contrib                                      # (c)
        _rejected(name + " moved", moved, d.ref)

    def mirror(level, f):                                            # (d)
        if level == c.levels - 1:
            f = f.copy()
            f[:, 0] = 1.0 - f[:, 0]
        return f
    lo, hi = int(d.offsets[c.levels - 1]), int(d.offsets[c.levels])
    swapped = good.copy()
    swapped[lo:hi] = grid_reference(d.g, d.x, d.emb, d.offsets, d.levels, c.gridtype, c.align,
                                    c.interp, frac_hook=mirror).ge[lo:hi].astype(np.float32)
    _rejected(name + " mirrored", swapped, d.ref)
    if c.interp == 1:                                                # (e)
        linear = grid_reference(d.g, d.x, d.emb, d.offsets, d.levels, c.gridtype, c.align, 0)
        _rejected(name + " linear weights", linear.ge.astype(np.float32), d.ref)


def test_reference_rows_known_answers(oracle_mod):
    """The integer row math against orc_grid_index on hand-picked points: dense, dense with
    the stride cut-off (tiled), hashed, align_corners, D = 2..5."""
    from tests.grid_ref import level_rows
    rng = np.random.default_rng(0)
    for D in (2, 3, 4, 5):
        for gridtype in (0, 1):
            for align in (False, True):
                for res, hsize in ((8, 88), (16, 4096), (64, 1 << 14), (256, 1 << 15)):
                    pl = rng.integers(0, res + 2, size=(64, D)).astype(np.int64)
                    got = level_rows(pl, res, hsize, gridtype, align)
                    want = [oracle_mod.grid_index(p, hsize, res, gridtype, align, C=1) for p in pl]
                    np.testing.assert_array_equal(got, want)

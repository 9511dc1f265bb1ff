"""The configurations, inputs and planning rule shared by test_grid_ref.py (CPU: the float64
reference against the C oracle on exactly these inputs) and test_gpu_grid_backward.py (the
HIP table gradient against the reference on every kernel path)."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from tests import grid_ref
from tests.golden import weights as W


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    C: int
    gridtype: int
    align: bool
    interp: int
    levels: int
    log2h: int
    B: int
    path: str                    # direct | windows | binned
    desired: int = 0             # 0: per-level scale 2
    one_point: bool = False


# (name, D, C, gridtype, align_corners, interpolation, levels, log2_hashmap_size, desired)
VARIANTS = [
    ("d2c4_smooth", 2, 4, 0, False, 1, 6, 12, 0),
    ("d3c1_tiled_align", 3, 1, 1, True, 0, 5, 13, 0),
    ("d3c8_align_smooth", 3, 8, 0, True, 1, 5, 15, 0),
    ("d4c2", 4, 2, 0, False, 0, 4, 14, 0),
    ("d5c2", 5, 2, 0, False, 0, 4, 15, 0),
    ("d3c2", 3, 2, 0, False, 0, 5, 15, 0),
    ("d3c2_res100", 3, 2, 0, False, 0, 5, 14, 100),      # non-integer scales
]


def _variant_cases():
    out = []
    for name, D, C, gt, ac, ip, L, h, des in VARIANTS:
        paths = [("direct", 255), ("direct", 4095), ("windows", 4097)]
        if D <= 3:
            paths.append(("binned", 4097))
        for path, B in paths:
            out.append(Case(f"{name}_{path}_{B}", D, C, gt, ac, ip, L, h, B, path, des))
    return out


VARIANT_CASES = _variant_cases()
# LDS-window edges: level 0 one window, level 1 two (the second partial), level 2 planned
# nine and filling four, levels 3 and 4 direct atomics
WINDOW_EDGES = Case("window_edges_c8", 3, 8, 0, False, 0, 5, 14, 16384, "windows")
# one level of 64 * bin_rows<C>() rows: every bin of it swept twice; the coarse levels'
# single bins (B * 8 entries) cut into several non-whole items
SECOND_SWEEP = [
    Case("second_sweep_c8", 3, 8, 0, False, 0, 4, 18, 16384, "binned"),
    Case("second_sweep_c4", 3, 4, 0, False, 0, 5, 19, 16384, "binned"),
    Case("second_sweep_c1", 3, 1, 0, False, 0, 5, 21, 16384, "binned"),
]
# 70 000 samples at one point: eight rows of the hashed two-sweep level receive more than
# the minimum chunk each, so their bins are split (whole == 0) and swept twice
ONE_POINT = Case("one_point_c8", 3, 8, 0, False, 0, 4, 18, 70000, "binned", one_point=True)

ALL_CASES = VARIANT_CASES + [WINDOW_EDGES] + SECOND_SWEEP + [ONE_POINT]
BY_NAME = {c.name: c for c in ALL_CASES}

BASE_RESOLUTION = 8


def make_inputs(case, seed):
    """Seeded uniform in [-0.02, 1.02]; four exact rows (all 0, 1, 0.5, 0.25: cell boundaries,
    where one weight is exactly zero, and the domain edges); the last eighth of the batch
    copies of one in-bounds sample.  The one-point case: one in-bounds point, |normal| g."""
    rng = np.random.default_rng(seed)
    B, D = case.B, case.D
    if case.one_point:
        x = np.tile(np.array([0.3, 0.55, 0.8, 0.45, 0.7][:D], np.float32), (B, 1))
    else:
        x = rng.uniform(-0.02, 1.02, size=(B, D)).astype(np.float32)
        x[0], x[1], x[2], x[3] = 0.0, 1.0, 0.5, 0.25
        inb = np.flatnonzero(np.all((x[4:] >= 0) & (x[4:] <= 1), axis=1))[0] + 4
        x[B - B // 8:] = x[inb]
    g = rng.normal(size=(case.levels, B, case.C)).astype(np.float32)
    if case.one_point:
        # same-sign gradients: ge = A, so the bound (~n A u) stays far below one lost work
        # item; with signed g the sum cancels to ~sqrt(n) and a lost item hides in the bound
        g = np.abs(g)
    return x, g


@functools.lru_cache(maxsize=2)
def case_data(name):
    """Inputs, table and float64 reference of a case, not to be modified.  Only the last two
    are kept (a reference holds four float64 tables): tests that share a case run next to
    each other."""
    from oracle import oracle
    c = BY_NAME[name]
    desired = c.desired or BASE_RESOLUTION * 2 ** (c.levels - 1)
    offsets, pls = oracle.grid_offsets(num_levels=c.levels, level_dim=c.C,
                                       base_resolution=BASE_RESOLUTION,
                                       log2_hashmap_size=c.log2h, desired_resolution=desired,
                                       input_dim=c.D, align_corners=c.align)
    S = np.float32(np.log2(pls))
    levels = oracle.level_table(c.levels, S, BASE_RESOLUTION, offsets)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    x, g = make_inputs(c, seed)
    emb = W.det_uniform((int(offsets[-1]), c.C), -1, 1, 17)
    ref = grid_ref.grid_reference(g, x, emb, offsets, levels, c.gridtype, c.align, c.interp)
    for a in (x, g, emb, offsets, ref.ge, ref.A, ref.G, ref.n, ref.sure, ref.fwd, ref.V, ref.vmax):
        a.setflags(write=False)
    return SimpleNamespace(case=c, offsets=offsets, pls=pls, S=float(S), levels=levels, x=x, g=g,
                           emb=emb, ref=ref)


# ---------------------------------------------------------------------------------------
# the kernel's planning rule (csrc/encoders.hip: window_levels, bin_levels, bin_shift,
# bin_chunk), restated so that every case can assert the path it is named for
# ---------------------------------------------------------------------------------------
LDS_BYTES = 128 * 1024
MAX_LEVEL_WINDOWS = 24
BIN_COUNT = 32
CHUNK_MIN, CHUNK_MAX = 1 << 16, 1 << 20
MIN_BATCH = 4096


def window_rows(C):
    return LDS_BYTES // 4 // C


def planned_windows(case, levels):
    """Windows planned per level, from (res (+1))^D + 8; 0: the level uses direct atomics."""
    out = []
    for _, res, _ in levels:
        need = math.ceil((float(res if case.align else res + 1) ** case.D + 8) / window_rows(case.C))
        out.append(need if case.B >= MIN_BATCH and need <= MAX_LEVEL_WINDOWS else 0)
    return out


def filled_windows(case, levels):
    return [math.ceil(h / window_rows(case.C)) for _, _, h in levels]


def bin_sweeps(case, hsize):
    """LDS sweeps over one bin of a level of hsize rows."""
    rows = window_rows(case.C)
    sh = rows.bit_length() - 1
    while (BIN_COUNT << sh) < hsize:
        sh += 1
    return (1 << sh) // rows


def bin_chunk(case):
    E = case.B * (1 << case.D) * case.levels
    return min(CHUNK_MAX, max(CHUNK_MIN, 2 * E // (case.levels * BIN_COUNT)))

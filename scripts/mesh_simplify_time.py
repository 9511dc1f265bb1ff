"""GPU mesh simplification against the host, on 1 GPU -> profiles/mesh_simplify_time.json.

The analytic sphere (radius 0.6 in network coordinates) through the sparse path
(``sparse_mesh``, as scripts/sparse_mesh_time.py runs it) at 512^3 and 1024^3, with
``simplify`` in {2, 4, 8}.  Per res:

  mesh         vertices and triangles of the full mesh, and the bytes its copy moves
  kernels      per k: the ``sdfr_mesh_simplify_count`` and ``_emit`` calls between device
               events (median and fastest of ``--reps`` runs after a warm-up), the counts, the
               workspace, and whether the result equals the NumPy definition
               (tests/mesh_simplify_ref.py; checked for ``--check-k`` only: the definition's
               duplicate pass is a Python loop over the faces)
  whole        ``sparse_mesh`` from the seeds to the ``Mesh`` on the host with simplify None,
               2, 4, 8: the arms alternate in one process after a warm-up run of each; host
               clock around a call that ends with the mesh on the host; median and fastest
               (the copy of the full mesh spreads by several ms from run to run), and the
               bytes copied
  host         the baseline: the copy of the full mesh to the host (median and fastest) plus
               the NumPy definition there (one run, ``--check-k``)

Default clocks (not pinned)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402
from tests import mesh_simplify_ref as S  # noqa: E402

DEV = "cuda:0"
RADIUS = 0.6


def sphere(sdfr, res):
    c = sdfr.cube_axis(res, DEV)
    axes = (c, -c, -c)

    def sdf(p):
        return p.norm(dim=-1) - RADIUS

    mid = torch.arange(res // 8, device=DEV) * 8 + 4
    centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"), -1)
    seeds = sdf(centres.reshape(-1, 3)).abs() <= 4 * 3 ** 0.5 * 2 / res      # L = 1
    return sdf, axes, seeds


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 3), fastest_ms=round(ms[0], 3), runs=len(ms))


def copied_bytes(n_vertices, n_faces):
    return 12 * n_vertices + 12 * n_faces          # fp32 [V, 3] and int32 [F, 3]


def time_kernels(sdfr, verts, faces, res, k, reps):
    """The two C calls between device events, as ``simplify_mesh`` issues them."""
    L = sdfr._lib
    lib = L.lib()
    V, F = verts.shape[0], faces.shape[0]
    n = lib.sdfr_mesh_simplify_workspace_bytes(V, F)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    counts = (L._u32 * 3)()
    st = L.stream_of(verts)
    dims = -(-res // k)
    out = None
    t_count, t_emit = [], []
    for r in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        L.check(lib.sdfr_mesh_simplify_count(L.ptr(verts), L.ptr(faces), V, F, 0.0, 0.0, 0.0,
                                             float(k), dims, dims, dims, 1, L.ptr(ws), n, counts,
                                             st), "count")
        e[1].record()
        nv, nf = int(counts[1]), int(counts[2])
        if out is None:
            out = (torch.empty(nv, 3, dtype=torch.float32, device=DEV),
                   torch.empty(nf, 3, dtype=torch.int32, device=DEV),
                   torch.empty(nv, dtype=torch.int32, device=DEV),
                   torch.empty(V, dtype=torch.int32, device=DEV),
                   torch.empty(nv, dtype=torch.int32, device=DEV))
        L.check(lib.sdfr_mesh_simplify_emit(L.ptr(verts), L.ptr(faces), V, F, nv, nf, L.ptr(ws),
                                            n, *(L.ptr(t) for t in out), st), "emit")
        e[2].record()
        torch.cuda.synchronize()
        if r:
            t_count.append(e[0].elapsed_time(e[1]))
            t_emit.append(e[1].elapsed_time(e[2]))
    row = dict(count=stats(t_count), emit=stats(t_emit), clusters=int(counts[0]),
               vertices=nv, triangles=nf, workspace_bytes=int(n),
               bytes_copied=copied_bytes(nv, nf))
    return row, out


def time_whole(sdfr, res, ks, reps):
    sdf, axes, seeds = sphere(sdfr, res)
    arms = [None] + list(ks)
    got = {k: [] for k in arms}
    sizes = {}
    for r in range(reps + 1):
        for k in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh = sdfr.sparse_mesh(sdf, axes, res, seeds, simplify=k)[0]
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if r:
                got[k].append(ms)
            sizes[k] = (len(mesh.vertices), len(mesh.faces))
            del mesh
    return {("none" if k is None else str(k)):
            dict(stats(got[k]), vertices=sizes[k][0], triangles=sizes[k][1],
                 bytes_copied=copied_bytes(*sizes[k])) for k in arms}


def time_host(verts, faces, res, k, reps):
    copies = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, f = verts.cpu().numpy(), faces.cpu().numpy()
        ms = (time.perf_counter() - t0) * 1e3
        if r:
            copies.append(ms)
    t0 = time.perf_counter()
    want = S.simplify(v, f, (0, 0, 0), float(k), (-(-res // k),) * 3)
    ref_ms = (time.perf_counter() - t0) * 1e3
    return dict(copy=stats(copies), k=k, numpy_definition_ms=round(ref_ms, 1),
                bytes_copied=copied_bytes(len(v), len(f))), want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--check-k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(REPO / "profiles" / "mesh_simplify_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_time.py needs the GPU")
    sdfr = load()
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
                  state="one process; a warm-up run of every arm, then the arms alternate; "
                        "kernels between device events, whole calls by the host clock around a "
                        "call that ends with the mesh on the host; default clocks (not pinned)",
                  field=f"analytic sphere, radius {RADIUS}", res={})
    for res in a.res:
        sdf, axes, seeds = sphere(sdfr, res)
        verts, faces, _ = sdfr.sparse_extract(sdf, axes, res, seeds)
        entry = dict(mesh=dict(vertices=int(len(verts)), triangles=int(len(faces)),
                               bytes_copied=copied_bytes(len(verts), len(faces))), kernels={})
        outs = {}
        for k in a.k:
            entry["kernels"][str(k)], outs[k] = time_kernels(sdfr, verts, faces, res, k, a.reps)
            print(res, k, json.dumps(entry["kernels"][str(k)]), flush=True)
        if a.check_k in outs:
            entry["host"], want = time_host(verts, faces, res, a.check_k, a.reps)
            got = [t.cpu().numpy() for t in outs[a.check_k]]
            same = (np.array_equal(got[0].view(np.uint32), want["verts"].view(np.uint32))
                    and all(np.array_equal(g, want[n]) for g, n in
                            zip(got[1:], ("faces", "index_map", "cluster", "members"))))
            entry["kernels"][str(a.check_k)]["equals_numpy_definition"] = bool(same)
            print(res, "host", json.dumps(entry["host"]), "equal", same, flush=True)
        del outs, verts, faces
        torch.cuda.empty_cache()
        entry["whole"] = time_whole(sdfr, res, a.k, a.reps)
        print(res, "whole", json.dumps(entry["whole"]), flush=True)
        result["res"][str(res)] = entry
        with open(a.out, "w") as f:                           # keep what is done so far
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""GPU mesh smoothing against the host, on 1 GPU -> profiles/mesh_smooth_time.json.

The analytic sphere (radius 0.6 in network coordinates) through the sparse path
(``sparse_extract``, as scripts/mesh_simplify_time.py runs it) at 1024^3: its full mesh and
its ``simplify=4`` result.  Per mesh:

  kernels      ``sdfr_mesh_smooth_prepare`` and ``sdfr_mesh_smooth_run`` between device events
               (median and fastest of ``--reps`` runs after a warm-up): prepare; a run of 20
               passes and one of 0 passes (the finish alone), whose difference / 20 is the time
               per pass; the pass's compulsory bytes (16 V state in, 16 V state out, 4 (V + 1)
               row offsets, 24 F rows -- the neighbours' state is a gather of 16-byte elements
               that are all in the state already counted) and the rate they give as a fraction
               of the 8 TB/s HBM figure of the renderer's gather roofline; 10 Taubin iterations
               end to end (prepare + run); whether the result equals the NumPy definition
  host         the copy of the mesh to the host (median and fastest) plus the NumPy definition
               there for the same 10 Taubin iterations (tests/mesh_smooth_ref.py, one run)

and ``sparse_mesh`` from the seeds to the ``Mesh`` on the host at 512^3 and 1024^3 with
``simplify`` None and 4, each with and without ``smooth=10``: the arms alternate in one process
after a warm-up run of each; host clock around a call that ends with the mesh on the host.
Then ``stages``: the steps of that call on the full 1024^3 mesh, plain and with ``smooth=10``
alternating, each by the host clock with a synchronisation after it (extraction, the
workspace from the caching allocator, ``smooth_mesh``, scaling, the two copies, the ``Mesh``
object), and the allocator's device allocations and frees per arm.

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
from tests import mesh_smooth_ref as M  # noqa: E402

DEV = "cuda:0"
RADIUS = 0.6
HBM_BYTES_PER_S = 8e12
PASSES = 20


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
    return dict(median_ms=round(ms[len(ms) // 2], 4), fastest_ms=round(ms[0], 4), runs=len(ms))


def time_kernels(sdfr, verts, faces, res, iterations, reps):
    """The two C calls between device events, as ``smooth_mesh`` issues them."""
    L = sdfr._lib
    lib = L.lib()
    V, F = verts.shape[0], faces.shape[0]
    origin, ul = sdfr.smooth_lattice((0, 0, 0), (res, res, res))
    n = lib.sdfr_mesh_smooth_workspace_bytes(V, F)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(verts)
    st = L.stream_of(verts)
    taubin = [0.5, -0.53] * iterations
    w_taubin = (L._f32 * len(taubin))(*taubin)
    w_passes = (L._f32 * PASSES)(*([0.5, -0.53] * (PASSES // 2)))
    t = dict(prepare=[], passes=[], finish=[], taubin=[])

    def prepare():
        L.check(lib.sdfr_mesh_smooth_prepare(L.ptr(verts), L.ptr(faces), V, F, *origin, ul, 1,
                                             L.ptr(ws), n, None, None, st), "prepare")

    def run(w, k):
        L.check(lib.sdfr_mesh_smooth_run(L.ptr(verts), V, w, k, L.ptr(ws), n, L.ptr(out), st),
                "run")

    for r in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record()
        prepare()
        e[1].record()
        run(w_passes, PASSES)
        e[2].record()
        run(w_passes, 0)
        e[3].record()
        torch.cuda.synchronize()
        e[4].record()
        prepare()
        run(w_taubin, len(taubin))
        e[5].record()
        torch.cuda.synchronize()
        if r:
            t["prepare"].append(e[0].elapsed_time(e[1]))
            t["passes"].append(e[1].elapsed_time(e[2]))
            t["finish"].append(e[2].elapsed_time(e[3]))
            t["taubin"].append(e[4].elapsed_time(e[5]))
    row = {k: stats(v) for k, v in t.items()}
    per_pass_ms = (row["passes"]["median_ms"] - row["finish"]["median_ms"]) / PASSES
    pass_bytes = 16 * V + 16 * V + 4 * (V + 1) + 24 * F
    row.update(passes_timed=PASSES, taubin_iterations=iterations,
               per_pass_ms=round(per_pass_ms, 4), pass_compulsory_bytes=pass_bytes,
               pass_bytes_per_s=round(pass_bytes / (per_pass_ms * 1e-3), 0),
               pass_fraction_of_hbm_8e12=round(pass_bytes / (per_pass_ms * 1e-3)
                                               / HBM_BYTES_PER_S, 3),
               workspace_bytes=int(n), vertices=int(V), triangles=int(F))
    return row, out, (origin, ul)


def time_host(verts, faces, lattice, iterations, reps):
    copies = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, f = verts.cpu().numpy(), faces.cpu().numpy()
        ms = (time.perf_counter() - t0) * 1e3
        if r:
            copies.append(ms)
    t0 = time.perf_counter()
    want = M.smooth(v, f, M.schedule(iterations), *lattice)
    ref_ms = (time.perf_counter() - t0) * 1e3
    return dict(copy=stats(copies), taubin_iterations=iterations,
                numpy_definition_ms=round(ref_ms, 1), bytes_copied=12 * len(v) + 12 * len(f)), want


def time_whole(sdfr, res, iterations, reps):
    sdf, axes, seeds = sphere(sdfr, res)
    arms = [(None, None), (None, iterations), (4, None), (4, iterations)]
    got = {a: [] for a in arms}
    sizes = {}
    for r in range(reps + 1):
        for a in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh = sdfr.sparse_mesh(sdf, axes, res, seeds, simplify=a[0], smooth=a[1])[0]
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if r:
                got[a].append(ms)
            sizes[a] = (len(mesh.vertices), len(mesh.faces))
            del mesh
    return {f"simplify={a[0]},smooth={a[1]}":
            dict(stats(got[a]), vertices=sizes[a][0], triangles=sizes[a][1]) for a in arms}


def time_stages(sdfr, res, iterations, reps):
    """Where the time of ``sparse_mesh`` on the full mesh goes, plain and smoothed: its own
    steps by the host clock with a synchronisation after each (so the sum exceeds the call's
    time, whose steps overlap), the two arms alternating as in ``time_whole``.  Also the
    caching allocator's device allocations and frees over the timed runs of each arm."""
    sdf, axes, seeds = sphere(sdfr, res)
    L = sdfr._lib
    lattice = sdfr.smooth_lattice((0.0,) * 3, (float(res),) * 3)
    names = ("extract", "workspace_alloc", "smooth_mesh", "scale", "copy_verts", "copy_faces",
             "mesh_object", "total")
    got = {arm: {n: [] for n in names} for arm in ("plain", "smooth")}
    allocs = {arm: [0, 0] for arm in got}

    def lap(t):
        torch.cuda.synchronize()
        now = time.perf_counter()
        return (now - t) * 1e3, now

    for r in range(reps + 1):
        for arm in got:
            before = torch.cuda.memory_stats()
            torch.cuda.synchronize()
            t = t0 = time.perf_counter()
            row = {}
            verts, faces, _ = sdfr.sparse_extract(sdf, axes, res, seeds)
            row["extract"], t = lap(t)
            if arm == "smooth":
                # (the workspace smooth_mesh is about to ask the caching allocator for)
                n = L.lib().sdfr_mesh_smooth_workspace_bytes(len(verts), len(faces))
                ws = torch.empty(n, dtype=torch.uint8, device=DEV)
                del ws
                row["workspace_alloc"], t = lap(t)
                verts = sdfr.smooth_mesh(verts, faces, iterations=iterations, origin=lattice[0],
                                         unit_log2=lattice[1]).verts
                row["smooth_mesh"], t = lap(t)
            for axis in range(3):
                verts[:, axis] = (verts[:, axis] / float(res) - 0.5) * 0.24
            verts[:, 2] *= -1
            verts[:, 1] *= -1
            row["scale"], t = lap(t)
            hv = verts.cpu().numpy()
            row["copy_verts"], t = lap(t)
            hf = faces.cpu().numpy()
            row["copy_faces"], t = lap(t)
            mesh = sdfr.Mesh(hv, hf)
            row["mesh_object"], t = lap(t)
            row["total"] = (t - t0) * 1e3
            del verts, faces, hv, hf, mesh
            after = torch.cuda.memory_stats()
            if r:
                for n, ms in row.items():
                    got[arm][n].append(ms)
                allocs[arm][0] += after["num_device_alloc"] - before["num_device_alloc"]
                allocs[arm][1] += after["num_device_free"] - before["num_device_free"]
    return {arm: dict({n: stats(ms) for n, ms in got[arm].items() if ms},
                      device_allocs=allocs[arm][0], device_frees=allocs[arm][1])
            for arm in got}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--whole-res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(REPO / "profiles" / "mesh_smooth_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_smooth_time.py needs the GPU")
    sdfr = load()
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
                  state="one process; a warm-up run of every arm, then the arms alternate; "
                        "kernels between device events, whole calls by the host clock around a "
                        "call that ends with the mesh on the host; default clocks (not pinned)",
                  field=f"analytic sphere, radius {RADIUS}", res=a.res, meshes={}, whole={})

    def save():
        with open(a.out, "w") as f:                               # keep what is done so far
            json.dump(result, f, indent=1)

    sdf, axes, seeds = sphere(sdfr, a.res)
    verts, faces, _ = sdfr.sparse_extract(sdf, axes, a.res, seeds)
    s = sdfr.simplify_mesh(verts, faces, cell=4.0, origin=(0.0, 0.0, 0.0),
                           dims=(-(-a.res // 4),) * 3)
    for name, (v, f) in (("full", (verts, faces)), ("simplify=4", (s.verts, s.faces))):
        row, out, lattice = time_kernels(sdfr, v, f, a.res, a.iterations, a.reps)
        print(name, json.dumps(row), flush=True)
        host, want = time_host(v, f, lattice, a.iterations, a.reps)
        row["equals_numpy_definition"] = bool(np.array_equal(
            out.cpu().numpy().view(np.uint32), want["verts"].view(np.uint32)))
        print(name, "host", json.dumps(host), "equal", row["equals_numpy_definition"], flush=True)
        result["meshes"][name] = dict(kernels=row, host=host)
        save()
    del verts, faces, s
    torch.cuda.empty_cache()
    for res in a.whole_res:
        result["whole"][str(res)] = time_whole(sdfr, res, a.iterations, a.reps)
        print(res, "whole", json.dumps(result["whole"][str(res)]), flush=True)
        save()
    result["stages"] = {str(a.res): time_stages(sdfr, a.res, a.iterations, a.reps)}
    print(a.res, "stages", json.dumps(result["stages"][str(a.res)]), flush=True)
    save()


if __name__ == "__main__":
    main()

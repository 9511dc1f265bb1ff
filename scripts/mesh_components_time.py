"""Mesh connected components on 1 GPU -> profiles/mesh_components_time.json.

Cases, through ``sparse_extract`` with analytic ``evaluate`` functions (no network): the
r = 0.6 sphere at 256^3, 512^3 and 1024^3 (one component), and a two-body volume at 512^3
(that sphere plus an r = 0.1 ball about (0.8, 0.8, 0.8), disjoint from it).

Per case, on the mesh as ``sparse_extract`` leaves it on the device (index coordinates):
device-event medians of ``label_components``, ``component_stats``, the selection
(``keep_components(largest=1)`` as a whole: label + stats + count + emit) and the copy of the
mesh to the host, with and without the filter; V, F and the bytes copied either way; and the
whole call -- ``sparse_mesh(...)``, the path of ``extract_mesh_sparse``, host clock around a
call that ends with the mesh on the host -- with ``components=None`` (the parent commit's
path, re-measured in this run) and with ``components={"largest": 1}``, alternating after a
warm-up run of each.  On the host: ``scipy.sparse.csgraph.connected_components`` of the same
mesh when scipy imports, else a vectorised NumPy min-label propagation, once.

Needs the GPU; default clocks (not pinned)."""
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

DEV = "cuda:0"
BALL = (0.8, 0.8, 0.8)


def sphere(p):
    return p.norm(dim=-1) - 0.6


def two_body(p):
    c = torch.tensor(BALL, device=p.device)
    return torch.minimum(p.norm(dim=-1) - 0.6, (p - c).norm(dim=-1) - 0.1)


def setup(sdfr, field, res):
    c = sdfr.cube_axis(res, DEV)
    axes = (c, -c, -c)
    nb = res // 8
    mid = torch.arange(nb, device=DEV) * 8 + 4
    centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"), -1)
    seeds = field(centres.reshape(-1, 3)).abs() <= 4 * 3 ** 0.5 * 2 / res        # L = 1
    return axes, seeds


def event_ms(fn, reps):
    """Median device-event time of fn() over reps runs after one warm-up run."""
    fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        del out
    return round(sorted(times)[len(times) // 2], 4)


def host_labels_numpy(faces, V):
    f = faces.astype(np.int64)
    e0 = np.concatenate([f[:, 0], f[:, 1]])
    e1 = np.concatenate([f[:, 1], f[:, 2]])
    label = np.arange(V, dtype=np.int64)
    while True:
        m = np.minimum(label[e0], label[e1])
        new = label.copy()
        np.minimum.at(new, e0, m)
        np.minimum.at(new, e1, m)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, label):
            return len(np.unique(label))
        label = new


def host_components(faces, V):
    """(method, ms, count) of the host baseline on faces [F, 3] (numpy)."""
    t0 = time.perf_counter()
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        count = host_labels_numpy(faces, V)
        return "numpy min-label propagation", (time.perf_counter() - t0) * 1e3, count
    t0 = time.perf_counter()
    rows = np.concatenate([faces[:, 0], faces[:, 1]])
    cols = np.concatenate([faces[:, 1], faces[:, 2]])
    g = sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)).tocsr()
    count, _ = connected_components(g, directed=False)
    return "scipy.sparse.csgraph.connected_components", (time.perf_counter() - t0) * 1e3, int(count)


def whole_call(sdfr, field, axes, res, seeds, components):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh, _ = sdfr.sparse_mesh(field, axes, res, seeds, components=components)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, mesh


def run_case(sdfr, name, field, res, reps):
    axes, seeds = setup(sdfr, field, res)
    verts, faces, _ = sdfr.sparse_extract(field, axes, res, seeds)
    V, F = len(verts), len(faces)
    row = dict(field=name, res=res, vertices=V, triangles=F)
    label, comp, count = sdfr.label_components(faces, V)
    row["components"] = count
    row["label_ms"] = event_ms(lambda: sdfr.label_components(faces, V), reps)
    row["stats_ms"] = event_ms(lambda: sdfr.component_stats(verts, faces, comp, count), reps)
    row["select_ms"] = event_ms(lambda: sdfr.keep_components(verts, faces, largest=1), reps)
    kv, kf, _ = sdfr.keep_components(verts, faces, largest=1)
    row["kept_vertices"], row["kept_triangles"] = len(kv), len(kf)
    row["copy_all_ms"] = event_ms(lambda: (verts.cpu(), faces.cpu()), reps)
    row["copy_kept_ms"] = event_ms(lambda: (kv.cpu(), kf.cpu()), reps)
    row["copied_bytes_all"] = 12 * V + 12 * F
    row["copied_bytes_kept"] = 12 * len(kv) + 12 * len(kf)
    method, ms, n = host_components(faces.cpu().numpy(), V)
    row["host_method"], row["host_ms"], row["host_components"] = method, round(ms, 2), n
    del label, comp, kv, kf, verts, faces
    torch.cuda.empty_cache()
    # the whole call, arms alternating after a warm-up run of each
    got = {"none": [], "largest1": []}
    arms = (("none", None), ("largest1", {"largest": 1}))
    for r in range(reps + 1):
        for arm, comps in arms:
            ms, mesh = whole_call(sdfr, field, axes, res, seeds, comps)
            if r:
                got[arm].append(ms)
            row[f"call_{arm}_triangles"] = int(len(mesh.faces))
            del mesh
    for arm, _ in arms:
        row[f"call_{arm}_ms"] = round(sorted(got[arm])[len(got[arm]) // 2], 3)
        row[f"call_{arm}_min_max_ms"] = [round(min(got[arm]), 3), round(max(got[arm]), 3)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sphere-res", type=int, nargs="*", default=[256, 512, 1024])
    ap.add_argument("--two-body-res", type=int, nargs="*", default=[512])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(REPO / "profiles" / "mesh_components_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_components_time.py needs the GPU")
    sdfr = load()
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
                  state="one process; per timed call one warm-up run, then the median of reps "
                        "runs; device events around label / stats / select / copies, host "
                        "clock around the whole call (ends with the mesh on the host), its "
                        "two arms alternating; default clocks (not pinned)", cases=[])
    cases = [("sphere", sphere, r) for r in a.sphere_res] + \
            [("two_body", two_body, r) for r in a.two_body_res]
    for name, field, res in cases:
        row = run_case(sdfr, name, field, res, a.reps)
        print(json.dumps(row), flush=True)
        result["cases"].append(row)
        with open(a.out, "w") as f:                       # keep what is done so far
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

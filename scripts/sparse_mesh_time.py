"""Dense against sparse meshing of the field itself, on 1 GPU -> profiles/sparse_mesh_time.json.

Dense is the earlier path: ``sdf_cube`` (the fused query on ``cube_points(res)``), then
``extract_mesh_with_marching_cubes``'s steps (dense marching cubes, vertex scaling and
flips, mesh copied to the host).  Sparse is ``extract_mesh_sparse``: the field on the
8^3-point bricks near the surface, csrc/mesh_sparse.hip, the same finish.  Both at the
median of a 64^3 cube's SDF (scripts/bench_mesh.py: a random-init SDF has no zero).

Fields: seeded random-init ngp and SIREN generators, and an analytic sphere (radius 0.6 in
network coordinates, through ``sparse_extract``) as the case of a surface that is a 2-D
set, which a random-init field's level set need not be.

Per res 128, 256, 512 the two arms alternate in one process after a warm-up run of each;
1024 runs sparse alone (dense marching cubes stops at 4 res^3 + 1 < 2^32).  Per row the
medians of total ms (host clock around a call that ends with the mesh on the host) and
field ms (device events around every field evaluation), their difference ("mc_ms": layout,
points, marching cubes, scaling, copies), peak allocated bytes, and the counts."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402

DEV = "cuda:0"


class Timed:
    """Wraps a field evaluation with device events; ``ms()`` sums and clears them."""

    def __init__(self, fn):
        self.fn, self.pairs = fn, []

    def __call__(self, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self.fn(*a, **kw)
        e1.record()
        self.pairs.append((e0, e1))
        return out

    def ms(self):
        torch.cuda.synchronize()
        total = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs = []
        return total


def finish(sdfr, verts, faces, res):
    for axis in range(3):
        verts[:, axis] = (verts[:, axis] / float(res) - 0.5) * 0.24
    verts[:, 2] *= -1
    verts[:, 1] *= -1
    return sdfr.Mesh(verts.cpu().numpy(), faces.cpu().numpy())


def network_field(sdfr, ngp):
    opt = sdfr.vol_render_opt(ngp=ngp)
    torch.manual_seed(0)
    g = sdfr.Generator(opt.model, opt.rendering, full_pipeline=False).to(DEV).eval()
    z = torch.randn(1, 256, device=DEV)
    with torch.no_grad():
        lat = g.styles_and_noise_forward([z])[0]
        level = float(sdfr.sdf_cube(g.renderer, lat, res=64).median())
    ren = g.renderer
    ren.query = Timed(ren.query)

    def dense(res):
        with torch.no_grad():
            cube = sdfr.sdf_cube(ren, lat, res=res)
        v, f = sdfr.marching_cubes(cube[0, ..., 0].permute(1, 0, 2), level)
        return finish(sdfr, v, f, res), {}

    def sparse(res):
        mesh, sv = sdfr.extract_mesh_sparse(ren, lat, res=res, level=level, return_volume=True)
        return mesh, dict(stored_fraction=sv.stored_fraction, rounds=sv.rounds,
                          n_bricks=sv.n_bricks)

    return dict(level=level, dense=dense, sparse=sparse, field_ms=ren.query.ms)


def sphere_field(sdfr, radius=0.6):
    def sdf(p):
        return p.norm(dim=-1) - radius
    ev = Timed(sdf)

    def dense(res):
        vol = ev(sdfr.cube_points(res, DEV)).permute(1, 0, 2)
        v, f = sdfr.marching_cubes(vol, 0.0)
        return finish(sdfr, v, f, res), {}

    def sparse(res):
        c = sdfr.cube_axis(res, DEV)
        axes = (c, -c, -c)
        nb = res // 8
        mid = torch.arange(nb, device=DEV) * 8 + 4
        centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"), -1)
        seeds = ev(centres.reshape(-1, 3)).abs() <= 4 * 3 ** 0.5 * 2 / res      # L = 1
        v, f, sv = sdfr.sparse_extract(ev, axes, res, seeds)
        return finish(sdfr, v, f, res), dict(stored_fraction=sv.stored_fraction,
                                              rounds=sv.rounds, n_bricks=sv.n_bricks)

    return dict(level=0.0, dense=dense, sparse=sparse, field_ms=ev.ms)


def run(field, arm, res):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    field["field_ms"]()
    t0 = time.perf_counter()
    mesh, extra = field[arm](res)
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    fms = field["field_ms"]()
    row = dict(total_ms=total, field_ms=fms, mc_ms=total - fms,
               peak_bytes=torch.cuda.max_memory_allocated(),
               vertices=int(len(mesh.vertices)), triangles=int(len(mesh.faces)), **extra)
    del mesh
    torch.cuda.empty_cache()
    return row


def median_row(rows):
    out = dict(rows[-1])
    for k in ("total_ms", "field_ms"):
        out[k] = round(sorted(r[k] for r in rows)[len(rows) // 2], 3)
    out["mc_ms"] = round(out["total_ms"] - out["field_ms"], 3)     # so that a row adds up
    out["runs"] = len(rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--sparse-only-res", type=int, nargs="*", default=[1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", nargs="+", default=["ngp", "siren", "sphere"])
    ap.add_argument("--out", default=str(REPO / "profiles" / "sparse_mesh_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_mesh_time.py needs the GPU")
    sdfr = load()
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
                  state="one process per run of the script; per res one warm-up run of each "
                        "arm, then the arms alternate; host clock around a call that ends "
                        "with the mesh on the host, device events around the field "
                        "evaluations; default clocks (not pinned)", fields={})
    for name in a.fields:
        field = sphere_field(sdfr) if name == "sphere" else network_field(sdfr, name == "ngp")
        rows = dict(level=field["level"])
        for res in a.res + a.sparse_only_res:
            arms = ("dense", "sparse") if res in a.res else ("sparse",)
            reps = a.reps if res < 512 else max(3, a.reps // 2)
            got = {arm: [] for arm in arms}
            try:
                for r in range(reps + 1):
                    for arm in arms:
                        row = run(field, arm, res)
                        if r:
                            got[arm].append(row)
            except ValueError as e:                       # e.g. too many bricks at 1024^3
                rows[str(res)] = dict(error=f"{type(e).__name__}: {e}"[:300])
                print(name, res, rows[str(res)], flush=True)
                torch.cuda.empty_cache()
                continue
            entry = {arm: median_row(v) for arm, v in got.items()}
            if len(arms) == 2:
                entry["same_counts"] = all(entry["dense"][k] == entry["sparse"][k]
                                           for k in ("vertices", "triangles"))
                entry["sparse_over_dense"] = round(entry["sparse"]["total_ms"]
                                                   / entry["dense"]["total_ms"], 3)
            rows[str(res)] = entry
            print(name, res, json.dumps(entry), flush=True)
            with open(a.out, "w") as f:                   # keep what is done so far
                json.dump(dict(result, fields=dict(result["fields"], **{name: rows})), f,
                          indent=1)
        result["fields"][name] = rows
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

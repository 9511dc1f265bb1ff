"""Time of the mesh rasteriser and of noise projection (profiling aid, not a test)
-> profiles/raster_time.json.

  raster     rasterize_mesh (sdfr_mesh_raster: project, scatter, resolve) plus one
             interpolate_vertex_attributes (sdfr_mesh_interpolate) of a one-channel attribute
             over a background, for the analytic sphere mesh of scripts/sparse_mesh_time.py at
             256^3 (radius 0.6 in network coordinates = 0.072 in world coordinates) as
             extracted and once subdivided, at 64^2, 128^2 and 256^2, for 1 and 8 views
  forward    Generator.forward at one face with the fixed noise maps (randomize_noise=False,
             graph_inference=False): plain, with project_noise (the maps formed up front,
             then the fused decoder) and with project_noise through the module path
             (use_fused=False: per-layer projection, op-by-op decoder)

One process; after two warm-up rounds (every arm, code objects loaded, clocks ramped by the
preceding rounds -- no clock pinning) the arms are interleaved in every round, device time by
events around each call; median, minimum and maximum over the rounds.  The raster arms'
kernels are then timed under torch.profiler in a run of their own (device time per call,
mean of 3 calls).
    python scripts/raster_time.py [--rounds 11] [--out profiles/raster_time.json]"""
import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402

DEV = "cuda:0"
KERNELS = ("raster_project_kernel", "raster_small_kernel", "raster_large_kernel",
           "raster_resolve_kernel", "mesh_interpolate_kernel")


def sphere_mesh(sdfr, res=256, radius=0.6):
    c = sdfr.cube_axis(res, DEV)
    axes = (c, -c, -c)
    nb = res // 8
    mid = torch.arange(nb, device=DEV) * 8 + 4
    centres = torch.stack(torch.meshgrid(*(a[mid] for a in axes), indexing="ij"), -1)
    sdf = lambda p: p.norm(dim=-1) - radius                                   # noqa: E731
    seeds = sdf(centres.reshape(-1, 3)).abs() <= 4 * 3 ** 0.5 * 2 / res
    v, f, _ = sdfr.sparse_extract(sdf, axes, res, seeds)
    for axis in range(3):
        v[:, axis] = (v[:, axis] / float(res) - 0.5) * 0.24
    v[:, 2] *= -1
    v[:, 1] *= -1
    return sdfr.Mesh(v.cpu().numpy(), f.cpu().numpy())


def timed_rounds(calls, rounds):
    times = {k: [] for k in calls}
    for rnd in range(rounds + 2):                                 # two warm-up rounds
        for name, fn in calls.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            if rnd >= 2:
                times[name].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "max_ms": round(max(v), 4)} for k, v in times.items()}


def kernel_times(fn, reps=3):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        kern = {}
        for ev in prof.key_averages():
            for k in KERNELS:
                if k in ev.key:
                    kern[k] = round(kern.get(k, 0.0) + ev.self_device_time_total / 1e3 / reps, 4)
        return kern
    except Exception as e:          # the record says so instead of carrying a guess
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=str(REPO / "profiles" / "raster_time.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 repetitions per arm")
    if not torch.cuda.is_available():
        raise SystemExit("raster_time.py needs the GPU")
    sdfr = load()
    rec = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "state": "one process, 2 warm-up rounds of every arm, arms interleaved per round, "
                    "device events around each call, default clocks (not pinned)"}
    meshes = {"extracted": sphere_mesh(sdfr)}
    meshes["subdivided"] = sdfr.subdivide_mesh(meshes["extracted"])
    rec["meshes"] = {k: {"vertices": int(len(m.vertices)), "triangles": int(len(m.faces))}
                     for k, m in meshes.items()}
    print(rec["meshes"], flush=True)

    # -- raster + resolve + one interpolation
    calls = {}
    for mname, mesh in meshes.items():
        attr = torch.randn(len(mesh.vertices), 1, device=DEV)
        for res in (64, 128, 256):
            for B in (1, 8):
                cam, focal, _, _, _ = sdfr.generate_camera_params(res, DEV, batch=B)
                bg = torch.randn(1, 1, res, res, device=DEV)

                def call(mesh=mesh, cam=cam, focal=focal, res=res, attr=attr, bg=bg):
                    r = sdfr.rasterize_mesh(mesh, cam, focal, res)
                    return r, sdfr.interpolate_vertex_attributes(mesh, r, attr, background=bg)

                calls[f"{mname}:{B}x{res}x{res}"] = call
    raster = timed_rounds(calls, a.rounds)
    for name, fn in calls.items():
        r, _ = fn()
        raster[name]["covered_fraction"] = round(float((r.face_idx >= 0).float().mean()), 4)
        raster[name]["kernels_ms_per_call"] = kernel_times(fn)
        print("raster", name, json.dumps(raster[name]), flush=True)
    rec["raster"] = raster

    # -- the cost of projection per frame
    opt = sdfr.vol_render_opt()
    opt.model.project_noise = True
    torch.manual_seed(0)
    g = sdfr.Generator(opt.model, opt.rendering).to(DEV).eval()
    g.graph_inference = False
    with torch.no_grad():
        for m in g.decoder.modules():
            if isinstance(m, sdfr.NoiseInjection):
                m.weight.fill_(0.1)
    z = torch.randn(1, 256, device=DEV)
    cam, focal, near, far, _ = sdfr.generate_camera_params(64, DEV, batch=1)
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "sphere.obj")
        meshes["extracted"].export(path)

        def forward(project, fused=True):
            g.decoder.use_fused = fused
            try:
                with torch.no_grad():
                    return g([z], cam, focal, near, far, randomize_noise=False,
                             project_noise=project, mesh_path=path if project else None)[0]
            finally:
                g.decoder.use_fused = True

        fwd = timed_rounds({"plain": lambda: forward(False),
                            "projected": lambda: forward(True),
                            "projected_module_path": lambda: forward(True, fused=False)},
                           a.rounds)
    fwd["projection_ms"] = round(fwd["projected"]["median_ms"] - fwd["plain"]["median_ms"], 4)
    fwd["module_over_fused"] = round(fwd["projected_module_path"]["median_ms"]
                                     / fwd["projected"]["median_ms"], 3)
    print("forward", json.dumps(fwd), flush=True)
    rec["forward"] = fwd
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Time of the fused FC field query and SDF gradient against the op-by-op module path they
replace (profiling aid, not a test): the FC golden weights, one face,
128^3 = 2 097 152 points (cube_points) each.  (The kernels' time does not depend on the
values: that these weights' late layers are nearly dead changes nothing here.)

  query_sdf        VolumeFeatureRenderer.query(return_rgb=False)   (sdfr_query_fc_forward)
  query_rgb        ... with a per-face direction and the colour
  gradient         VolumeFeatureRenderer.query_gradient            (sdfr_query_fc_grad)
  module_query_sdf / module_query_rgb / module_gradient
                   the same three Python calls with use_fused = False: the positional
                   encodings, nine linear + ReLU ops and the heads (and autograd for the
                   gradient) -- the path these calls took before the fused kernels existed,
                   the baseline.  Run in chunks of 2^18 points so
                   the [points, 256] activations and their backward fit in memory.
  central_diff     six fused query(return_rgb=False) calls at p +- h e_k (the arithmetic to
                   combine them is not counted)
  render           for scale: the fused 128^2 x 128 frustum render of one face
                   (sdfr_render_fc_forward, as many samples as the cube has points)

One process; after two warm-up rounds (every shape, code objects loaded, clocks ramped by
the preceding rounds -- no clock pinning) the arms are interleaved in every round, device
time by events around each call; median and minimum over the rounds.
    python scripts/fc_query_time.py [--rounds 11] [--out profiles/fc_query_time.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402
from tests.golden import weights as W  # noqa: E402


def make_renderer(sdfr, sd, res, N, dev):
    opt = sdfr.vol_render_opt(ngp=False, fc=True)
    r = opt.rendering
    r.N_samples = N
    r.return_sdf = True
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res)
    own = ren.state_dict()
    ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()
                         if k[len("renderer."):] in own}, strict=True)
    return ren.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--module-chunk", type=int, default=1 << 18)
    ap.add_argument("--out", default=str(REPO / "profiles" / "fc_query_time.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 repetitions per arm")
    sdfr = load()
    dev = "cuda:0"
    res = a.res
    golden = REPO / "tests" / "golden"
    sd = W.det_state_dict(W.golden_entries(golden, kind="fc"), "renderer.")
    ren = make_renderer(sdfr, sd, 8, 24, dev)
    frustum = make_renderer(sdfr, sd, res, res, dev)
    lat = torch.from_numpy(np.load(golden / "render_fc_small.npz")["latent"][:1]).to(dev)
    pts = sdfr.cube_points(res, dev).reshape(1, -1, 3).contiguous()
    view = torch.tensor([[0.0, 0.0, -1.0]], device=dev)
    h = 1.0 / 4096
    shifted = [(pts + s * h * torch.eye(3, device=dev)[k]).contiguous()
               for k in range(3) for s in (1.0, -1.0)]
    torch.manual_seed(0)
    cam, focal, near, far, _ = sdfr.generate_camera_params(res, dev, batch=1)
    t_rand = torch.rand(1, res, res)
    with torch.no_grad():
        assert ren._query_fused_ok(pts, lat) and frustum._fused_ok(cam, lat, False)

    def fused(fn):
        def run():
            with torch.no_grad():
                return fn(pts)
        return run

    def module(fn):
        def run():
            ren.use_fused = False
            try:
                with torch.no_grad():
                    return [fn(pts[:, m0:m0 + a.module_chunk].contiguous())
                            for m0 in range(0, pts.shape[1], a.module_chunk)]
            finally:
                ren.use_fused = True
        return run

    q_sdf = lambda p: ren.query(p, lat, return_rgb=False)  # noqa: E731
    q_rgb = lambda p: ren.query(p, lat, viewdirs=view)  # noqa: E731
    grad = lambda p: ren.query_gradient(p, lat)  # noqa: E731

    def central_diff():
        with torch.no_grad():
            return [ren.query(p, lat, return_rgb=False)[0] for p in shifted]

    def render():
        with torch.no_grad():
            return frustum(cam, focal, near, far, styles=lat, t_rand=t_rand)

    calls = {"query_sdf": fused(q_sdf), "query_rgb": fused(q_rgb), "gradient": fused(grad),
             "module_query_sdf": module(q_sdf), "module_query_rgb": module(q_rgb),
             "module_gradient": module(grad), "central_diff": central_diff, "render": render}
    times = {k: [] for k in calls}
    for rnd in range(a.rounds + 2):                           # two warm-up rounds
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            if rnd >= 2:
                times[name].append(e0.elapsed_time(e1))
    points = res ** 3
    rec = {"points": points, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "state": "one process, 2 warm-up rounds of every arm, arms interleaved per round, "
                    "device events around each call, default clocks (not pinned)",
           "module_chunk_points": a.module_chunk}
    for name, v in times.items():
        med = statistics.median(v)
        rec[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "ns_per_point_median": round(med * 1e6 / points, 3)}
        print(f"{name:17s} median {med:9.3f} ms  min {min(v):9.3f} ms  "
              f"{med * 1e6 / points:7.2f} ns/point")
    for k in ("query_sdf", "query_rgb", "gradient"):
        rec[f"module_over_fused_{k}"] = round(rec[f"module_{k}"]["median_ms"] /
                                              rec[k]["median_ms"], 3)
        print(f"module / fused {k}: {rec[f'module_over_fused_{k}']:.2f}")
    rec["central_diff_over_gradient"] = round(rec["central_diff"]["median_ms"] /
                                              rec["gradient"]["median_ms"], 3)
    print(f"central_diff / gradient {rec['central_diff_over_gradient']:.2f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

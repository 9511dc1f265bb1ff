"""Time of the fused field query against the two ways the same samples were evaluated
before it (profiling aid, not a test), one face, 128^3 = 2 097 152 samples each:

  query    VolumeFeatureRenderer.query on cube_points(128), one direction per face
           (sdfr_query_ngp_forward, SDF + colour)
  render   the frustum render sdf_mesh.py uses: 128^2 rays x 128 samples with return_sdf
           (sdfr_render_ngp_forward: the same gather and field kernel + compositing)
  module   renderer.network on the query's points, op by op (PyTorch-ROCm GEMMs, HIP
           encoders) -- the only way to ask for the colour at a point before the query

One process, the three interleaved in every round (clock and cache state shared), device
time by events around each call; median and minimum over the rounds.
    python scripts/query_time.py [--rounds 9] [--out profiles/query_time.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--out", default=str(REPO / "profiles" / "query_time.json"))
    a = ap.parse_args()
    sdfr = load()
    dev = "cuda:0"
    res = a.res
    opt = sdfr.vol_render_opt()
    r = opt.rendering
    r.N_samples = res
    r.return_sdf = True
    torch.manual_seed(0)
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res).to(dev).eval()
    ren.rng_device = "device"
    lat = torch.randn(1, 256, device=dev)
    ext, focal, near, far, _ = sdfr.generate_camera_params(res, dev, batch=1)
    pts = sdfr.cube_points(res, dev).reshape(1, -1, 3).contiguous()
    d = torch.tensor([[0.0, 0.0, -1.0]], device=dev)
    full = torch.cat([pts, d[:, None].expand_as(pts)], -1)

    calls = {
        "query": lambda: ren.query(pts, lat, viewdirs=d),
        "query_sdf_only": lambda: ren.query(pts, lat, return_rgb=False),
        "render": lambda: ren(ext, focal, near, far, styles=lat),
        "module": lambda: ren.network(full, styles=lat),
    }
    times = {k: [] for k in calls}
    with torch.no_grad():
        for rnd in range(a.rounds + 2):                       # two warm-up rounds
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                del out
                if rnd >= 2:
                    times[name].append(e0.elapsed_time(e1))
    samples = res ** 3
    rec = {"samples": samples, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for name, v in times.items():
        med = statistics.median(v)
        rec[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "ns_per_sample_median": round(med * 1e6 / samples, 3)}
        print(f"{name:15s} median {med:9.3f} ms  min {min(v):9.3f} ms  "
              f"{med * 1e6 / samples:7.2f} ns/sample")
    rec["query_over_render"] = round(rec["query"]["median_ms"] / rec["render"]["median_ms"], 4)
    rec["module_over_query"] = round(rec["module"]["median_ms"] / rec["query"]["median_ms"], 3)
    print(f"query / render {rec['query_over_render']:.3f}   module / query "
          f"{rec['module_over_query']:.2f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

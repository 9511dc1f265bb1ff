"""Time of the fused SDF gradient against the two ways to get a gradient of the ngp field
without it (profiling aid, not a test), one face, 128^3 = 2 097 152 points each:

  gradient      VolumeFeatureRenderer.query_gradient on cube_points(128)
                (sdfr_query_ngp_grad: SDF + exact gradient)
  central_diff  six fused query(return_rgb=False) calls at p +- h e_k: the central
                difference a user would write without the gradient call (its arithmetic to
                combine them is not counted)
  autograd      torch.autograd.grad through renderer.network, op by op, in chunks of
                2^18 points so the [S,256] activations and their backward fit in memory

One process; after two warm-up rounds (every shape, code objects loaded, clocks ramped by
the preceding rounds -- no clock pinning) the three are interleaved in every round, device
time by events around each call; median and minimum over the rounds.
    python scripts/gradient_time.py [--rounds 11] [--out profiles/gradient_time.json]"""
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
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--autograd-chunk", type=int, default=1 << 18)
    ap.add_argument("--out", default=str(REPO / "profiles" / "gradient_time.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 repetitions per arm")
    sdfr = load()
    dev = "cuda:0"
    res = a.res
    opt = sdfr.vol_render_opt()
    r = opt.rendering
    r.return_sdf = True
    torch.manual_seed(0)
    ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=8).to(dev).eval()
    lat = torch.randn(1, 256, device=dev)
    pts = sdfr.cube_points(res, dev).reshape(1, -1, 3).contiguous()
    h = 1.0 / 4096
    shifted = [(pts + s * h * torch.eye(3, device=dev)[k]).contiguous()
               for k in range(3) for s in (1.0, -1.0)]

    def gradient():
        with torch.no_grad():
            return ren.query_gradient(pts, lat)

    def central_diff():
        with torch.no_grad():
            return [ren.query(p, lat, return_rgb=False)[0] for p in shifted]

    def autograd():
        out = []
        for m0 in range(0, pts.shape[1], a.autograd_chunk):
            p = pts[:, m0:m0 + a.autograd_chunk].clone().requires_grad_(True)
            raw = ren.network(torch.cat([p, torch.zeros_like(p)], -1), styles=lat)
            out.append(torch.autograd.grad(raw[..., 3].sum(), p)[0])
        return out

    calls = {"gradient": gradient, "central_diff": central_diff, "autograd": autograd}
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
           "autograd_chunk_points": a.autograd_chunk}
    for name, v in times.items():
        med = statistics.median(v)
        rec[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                     "ns_per_point_median": round(med * 1e6 / points, 3)}
        print(f"{name:13s} median {med:9.3f} ms  min {min(v):9.3f} ms  "
              f"{med * 1e6 / points:7.2f} ns/point")
    g = rec["gradient"]["median_ms"]
    rec["central_diff_over_gradient"] = round(rec["central_diff"]["median_ms"] / g, 3)
    rec["autograd_over_gradient"] = round(rec["autograd"]["median_ms"] / g, 3)
    print(f"central_diff / gradient {rec['central_diff_over_gradient']:.2f}   "
          f"autograd / gradient {rec['autograd_over_gradient']:.2f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

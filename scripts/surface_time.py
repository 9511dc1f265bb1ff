"""Time of the fused surface render against the routes to the same result without it
(profiling aid, not a test), for the ngp and the SIREN network at 32 faces of 64^2 x 24
samples and at 1 face of 128^2 x 128 (sdf_mesh.py's surface shape):

  surface    VolumeFeatureRenderer.render_surface(refine_steps=8) with every output
             (sdfr_render_{ngp,siren}_surface)
  composed   the same result from the public calls that existed before it:
             forward(return_sdf=True), torch ops for the bracket and the bisection steps,
             query per step, query_gradient and query at the hit points
  module     _module_surface: the definition op by op on renderer.network
  render     the plain fused render (rgb + features + sdf), for scale

One process; after two warm-up rounds (every shape, code objects loaded, clocks ramped by the
preceding rounds -- no clock pinning) the arms are interleaved in every round, device time by
events around each call; median, minimum and maximum over the rounds.  The surface call's
kernels are then timed under torch.profiler in a run of their own (device time per call,
mean of 3 calls).
    python scripts/surface_time.py [--rounds 11] [--out profiles/surface_time.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402

ALL = ("hit", "sample", "depth", "xyz", "normal", "rgb", "residual", "sdf")
KERNELS = ("geom_points_kernel", "query_geom_kernel", "ngp_encode_kernel", "field_r_kernel",
           "field_p_kernel", "ngp_encode_grad_kernel", "field_g_kernel", "xprep_kernel",
           "surf_bracket_kernel", "surf_step_kernel", "surf_hit_kernel", "surf_maps_kernel")
K = 8


def composed(ren, cam, focal, near, far, lat, tr):
    """render_surface's result from forward, query and query_gradient plus torch glue."""
    B, res, N = cam.shape[0], ren.out_im_res, ren.N_samples
    sdf = ren(cam, focal, near, far, styles=lat, t_rand=tr)[2][..., 0]
    rays_o, rays_d, viewdirs, nr, fr = ren.camera_rays(focal, cam, near, far)
    z_vals = ren.sample_points(rays_o, rays_d, nr, fr, tr, ren._stratify())[0].expand(sdf.shape)
    span = fr - nr
    cross = (sdf[..., :-1] > 0) & (sdf[..., 1:] <= 0)
    steps = torch.arange(N - 1, device=sdf.device).expand(cross.shape)
    first = torch.where(cross, steps, torch.full_like(steps, N)).min(-1).values
    hit = first < N
    s0 = torch.where(hit, first, torch.zeros_like(first)).unsqueeze(-1)
    a, b = z_vals.gather(-1, s0)[..., 0], z_vals.gather(-1, s0 + 1)[..., 0]
    fa, fb = sdf.gather(-1, s0)[..., 0], sdf.gather(-1, s0 + 1)[..., 0]

    def net_point(z):
        p = rays_o + rays_d * z.unsqueeze(-1)
        return p, (p * 2 / span if ren.z_normalize else p).reshape(B, -1, 3)

    for _ in range(K):
        m = 0.5 * (a + b)
        f = ren.query(net_point(m)[1], lat, return_rgb=False)[0].reshape(a.shape)
        pos = f > 0
        a, fa = torch.where(pos, m, a), torch.where(pos, f, fa)
        b, fb = torch.where(pos, b, m), torch.where(pos, fb, f)
    t = torch.where(hit, fa / (fa - fb), torch.zeros_like(fa))
    z = torch.minimum(torch.maximum(a + t * (b - a), a), b)
    p, pn = net_point(z)
    res_sdf, g = ren.query_gradient(pn, lat)
    e = g.reshape(p.shape) * 2 / span if ren.z_normalize else g.reshape(p.shape)
    normal = e / e.norm(dim=-1, keepdim=True).clamp_min(1e-20)
    rgb = ren.query(pn, lat, viewdirs=viewdirs.reshape(B, -1, 3).contiguous())[1]
    mask = hit.unsqueeze(1)
    nchw = lambda v: torch.where(mask, v.reshape(B, res, res, -1).permute(0, 3, 1, 2),  # noqa: E731
                                 torch.zeros((), device=v.device)).contiguous()
    return (mask.float(), torch.where(hit, first, -torch.ones_like(first)).int().unsqueeze(1),
            nchw(z), nchw(p), nchw(normal), nchw(rgb), nchw(res_sdf), sdf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=str(REPO / "profiles" / "surface_time.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 repetitions per arm")
    sdfr = load()
    dev = "cuda:0"
    rec = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0), "refine_steps": K,
           "state": "one process, 2 warm-up rounds of every arm, arms interleaved per round, "
                    "device events around each call, default clocks (not pinned); randomly "
                    "initialised networks (the call's cost does not depend on the values)",
           "shapes": {}}
    for net in ("ngp", "siren"):
        for B, res, N in ((32, 64, 24), (1, 128, 128)):
            opt = sdfr.vol_render_opt(ngp=net == "ngp")
            r = opt.rendering
            r.N_samples = N
            r.return_sdf = True
            torch.manual_seed(0)
            ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res).to(dev).eval()
            for p in ren.parameters():
                p.requires_grad_(False)
            cam, focal, near, far, _ = sdfr.generate_camera_params(res, dev, batch=B)
            lat = torch.randn(B, 256, device=dev)
            tr = torch.rand(B, res, res, device=dev)
            args = (cam, focal, near, far, lat)

            def surface():
                with torch.no_grad():
                    return ren.render_surface(*args, t_rand=tr, refine_steps=K, want=ALL)

            def composed_():
                with torch.no_grad():
                    return composed(ren, *args, tr)

            def module():
                ren.use_fused = False
                try:
                    with torch.no_grad():
                        return ren.render_surface(*args, t_rand=tr, refine_steps=K, want=ALL)
                finally:
                    ren.use_fused = True

            def render():
                with torch.no_grad():
                    return ren(*args[:4], styles=lat, t_rand=tr)

            assert ren._query_fused_ok(cam, lat) and ren._fused_ok(cam, lat, False)
            calls = {"surface": surface, "composed": composed_, "module": module,
                     "render": render}
            times = {k: [] for k in calls}
            for rnd in range(a.rounds + 2):                       # two warm-up rounds
                for name, fn in calls.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd == 0 and name == "surface":
                        hit_fraction = float(out.hit.mean())
                    del out
                    if rnd >= 2:
                        times[name].append(e0.elapsed_time(e1))
            points = B * res * res * N
            shape = {"net": net, "faces": B, "res": res, "samples_per_ray": N, "points": points,
                     "hit_fraction": round(hit_fraction, 4)}
            for name, v in times.items():
                med = statistics.median(v)
                shape[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                               "max_ms": round(max(v), 4)}
                print(f"{net} {B}x{res}^2x{N} {name:9s} median {med:9.3f} ms  "
                      f"min {min(v):9.3f}  max {max(v):9.3f}")
            s = shape["surface"]["median_ms"]
            shape["composed_over_surface"] = round(shape["composed"]["median_ms"] / s, 3)
            shape["module_over_surface"] = round(shape["module"]["median_ms"] / s, 3)
            shape["surface_over_render"] = round(s / shape["render"]["median_ms"], 3)
            try:
                from torch.profiler import ProfilerActivity, profile
                reps = 3
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    for _ in range(reps):
                        surface()
                    torch.cuda.synchronize()
                kern = {}
                for ev in prof.key_averages():
                    for k in KERNELS:
                        if k in ev.key:
                            kern[k] = round(kern.get(k, 0.0)
                                            + ev.self_device_time_total / 1e3 / reps, 4)
                shape["kernels_ms_per_call"] = kern
                print(f"{net} {B}x{res}^2x{N} kernels (ms per render_surface): {kern}")
            except Exception as e:  # the record says so instead of carrying a guess
                shape["kernels_ms_per_call"] = None
                shape["kernels_error"] = repr(e)
            rec["shapes"][f"{net}:{B}x{res}x{res}x{N}"] = shape
            del ren
            torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Time of the fused geometry render against the only route to the same outputs without it
(profiling aid, not a test), at 32 faces of 64^2 x 24 samples and at 1 face of 128^2 x 128
(sdf_mesh.py's surface shape):

  geometry   VolumeFeatureRenderer.render_geometry with every output
             (sdfr_render_ngp_geometry: sample points, gradient gather, forward-mode field
             kernel, compositing kernel)
  autograd   forward(..., return_eikonal=True) with return_sdf / return_xyz under
             enable_grad, op by op (faces in chunks of at most --autograd-chunk points so
             the [S,256] activations and the double-backward graph fit in memory), plus the
             torch ops that rebuild the sampler's depths and the compositing weights and
             form the normal and depth maps
  render     the plain fused render (rgb + features + sdf + xyz + mask), for scale

One process; after two warm-up rounds (every shape, code objects loaded, clocks ramped by the
preceding rounds -- no clock pinning) the three are interleaved in every round, device time
by events around each call; median and minimum over the rounds.  The geometry call's kernels
are then timed on their own under torch.profiler (device time per call, mean of 3 calls).
    python scripts/geometry_time.py [--rounds 11] [--out profiles/geometry_time.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from sdfr_loader import load  # noqa: E402

ALL = ("normal", "depth", "xyz", "mask", "sdf", "eikonal")
KERNELS = ("geom_points_kernel", "ngp_encode_grad_kernel", "field_g_kernel",
           "geom_composite_kernel")


def _weights(ren, sdf, z_vals, rays_d):
    """volume_integration's weights from its returned per-sample SDF (torch ops)."""
    dists = z_vals[..., 1:] - z_vals[..., :-1]
    dn = torch.norm(rays_d.unsqueeze(3), dim=-1)
    dists = torch.cat([dists, ren.inf.expand(dn.shape)], -1) * dn
    sigma = 1 - torch.exp(-ren.sdf_activation(-sdf) * dists.unsqueeze(-1))
    vis = torch.cumprod(torch.cat([torch.ones_like(sigma[..., :1, :]), 1. - sigma + 1e-10], 3),
                        3)[..., :-1, :]
    w = sigma * vis
    if ren.force_background:
        w[..., -1, :] = 1 - w[..., :-1, :].sum(3)
    return w


def _depths(ren, cam, focal, near, far, t_rand):
    """The sampler's z-values and ray directions, as render_rays forms them."""
    _, rays_d, _ = ren.get_rays(focal, cam)
    nr, fr = near.reshape(-1, 1, 1, 1), far.reshape(-1, 1, 1, 1)
    z = nr * (1. - ren.t_vals) + fr * ren.t_vals
    z = z.expand(cam.shape[0], ren.out_im_res, ren.out_im_res, -1)
    if ren.perturb > 0:
        upper = torch.cat([z[..., 1:], fr.expand_as(z[..., :1])], -1)
        z = z + (upper - z) * t_rand.unsqueeze(-1)
    return z, rays_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--autograd-chunk", type=int, default=1 << 19)
    ap.add_argument("--out", default=str(REPO / "profiles" / "geometry_time.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 repetitions per arm")
    sdfr = load()
    dev = "cuda:0"
    rec = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "state": "one process, 2 warm-up rounds of every arm, arms interleaved per round, "
                    "device events around each call, default clocks (not pinned)",
           "autograd_chunk_points": a.autograd_chunk, "shapes": {}}
    for B, res, N in ((32, 64, 24), (1, 128, 128)):
        opt = sdfr.vol_render_opt()
        r = opt.rendering
        r.N_samples = N
        r.return_sdf = True
        r.return_xyz = True
        torch.manual_seed(0)
        ren = sdfr.VolumeFeatureRenderer(r, style_dim=256, out_im_res=res).to(dev).eval()
        for p in ren.parameters():
            p.requires_grad_(False)
        cam, focal, near, far, _ = sdfr.generate_camera_params(res, dev, batch=B)
        lat = torch.randn(B, 256, device=dev)
        tr = torch.rand(B, res, res, device=dev)
        per_face = res * res * N
        faces = max(1, a.autograd_chunk // per_face)

        def geometry():
            with torch.no_grad():
                return ren.render_geometry(cam, focal, near, far, lat, t_rand=tr, want=ALL)

        def autograd():
            out = []
            with torch.enable_grad():
                for b0 in range(0, B, faces):
                    s = slice(b0, b0 + faces)
                    _, _, sdf, mask, xyz, eik = ren(cam[s], focal[s], near[s], far[s],
                                                    styles=lat[s], return_eikonal=True,
                                                    t_rand=tr[s])
                    sdf, eik = sdf.detach(), eik.detach()
                    z, rays_d = _depths(ren, cam[s], focal[s], near[s], far[s], tr[s])
                    w = _weights(ren, sdf, z, rays_d)
                    normal = torch.sum(w * eik, 3).permute(0, 3, 1, 2).contiguous()
                    depth = torch.sum(w * z.unsqueeze(-1), 3).permute(0, 3, 1, 2).contiguous()
                    out.append((normal, depth, xyz.detach(), mask.detach(), sdf, eik))
            return out

        def render():
            with torch.no_grad():
                return ren(cam, focal, near, far, styles=lat, t_rand=tr)

        assert ren._query_fused_ok(cam, lat) and ren._fused_ok(cam, lat, False)
        assert not ren._fused_ok(cam, lat, True)
        calls = {"geometry": geometry, "autograd": autograd, "render": render}
        times = {k: [] for k in calls}
        for rnd in range(a.rounds + 2):                           # two warm-up rounds
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
        points = B * per_face
        # render_geometry's chunking: whole faces per call, or bands of whole rows
        chunk = ren.GRADIENT_CHUNK_POINTS
        if per_face <= chunk:
            calls_per_geometry = -(-B // (chunk // per_face))
        else:
            calls_per_geometry = B * -(-res // max(1, chunk // (res * N)))
        shape = {"faces": B, "res": res, "samples_per_ray": N, "points": points,
                 "autograd_faces_per_chunk": faces,
                 "geometry_calls": calls_per_geometry}
        for name, v in times.items():
            med = statistics.median(v)
            shape[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                           "ns_per_point_median": round(med * 1e6 / points, 3)}
            print(f"{B}x{res}^2x{N} {name:9s} median {med:9.3f} ms  min {min(v):9.3f} ms  "
                  f"{med * 1e6 / points:7.2f} ns/point")
        g = shape["geometry"]["median_ms"]
        shape["autograd_over_geometry"] = round(shape["autograd"]["median_ms"] / g, 3)
        shape["geometry_over_render"] = round(g / shape["render"]["median_ms"], 3)
        # the call's kernels on their own
        try:
            from torch.profiler import ProfilerActivity, profile
            reps = 3
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    geometry()
                torch.cuda.synchronize()
            kern = {}
            for ev in prof.key_averages():
                for k in KERNELS:
                    if k in ev.key:
                        kern[k] = round(kern.get(k, 0.0) + ev.self_device_time_total / 1e3 / reps, 4)
            shape["kernels_ms_per_call"] = kern
            print(f"{B}x{res}^2x{N} kernels (ms per render_geometry): {kern}")
        except Exception as e:  # the record says so instead of carrying a guess
            shape["kernels_ms_per_call"] = None
            shape["kernels_error"] = repr(e)
        rec["shapes"][f"{B}x{res}x{res}x{N}"] = shape
        del ren
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

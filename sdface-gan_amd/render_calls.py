"""The renderer's calls into libsdfr: what ``VolumeFeatureRenderer`` (renderer.py) needs to
run its fused paths -- the render, the point query, the SDF gradient, the geometry and the
surface render (include/sdfr.h) -- on the C ABI: argument structs, weight packing caches,
chunking and workspaces.  ``FusedCalls`` is the mixin the renderer inherits; the module
functions build the structs (ops.py uses them for the registered op sdfr::render_fused).
The three networks are told apart by ``kind``, the index into ``_lib.NETWORKS``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


def _per_face(x, B, device):
    t = torch.as_tensor(x, dtype=torch.float32, device=device).reshape(-1)
    return (t.expand(B) if t.numel() == 1 else t).contiguous()


def _workspace(ws, need, device):
    """``ws`` if it holds ``need`` bytes, else a new one that does."""
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


# struct member -> (name, index | None) once, for weights_struct and _weight_tensors
_SLOTS = tuple(tuple((f[:-3], int(f[-2])) if f.endswith("]") else (f, None) for f in n.fields)
               for n in _lib.NETWORKS)


def weights_struct(kind, ts, fscal, iscal, with_sdf: bool):
    """sdfr_{ngp,siren,fc}_weights from the flat tensor list of ``_weight_tensors`` (in the
    order of ``_lib.NETWORKS[kind].fields``) and the network's scalars (ngp: fscal = (log2
    per-level scale, bound), iscal = (base resolution,); SIREN / FC: iscal = (depth,
    width))."""
    w = _lib.NETWORKS[kind].weights()
    for (name, i), t in zip(_SLOTS[kind], ts, strict=True):
        if i is None:
            setattr(w, name, t.data_ptr())
        else:
            getattr(w, name)[i] = t.data_ptr()
    if kind == 0:
        w.num_levels = ts[1].shape[0] - 1
        w.log2_per_level_scale, w.bound = float(fscal[0]), float(fscal[1])
        w.base_resolution = int(iscal[0])
    else:
        w.depth, w.width = int(iscal[0]), int(iscal[1])
    if not with_sdf:
        w.sigmoid_beta = None
    return w


CAMERA_FLAGS = ("offset_sampling", "static_viewdirs", "z_normalize", "force_background")


def camera_args(a, inputs, H, W, N, flags, band=None):
    """The camera and sampling members that sdfr_ngp_render_args, sdfr_ngp_geometry_args and
    sdfr_surface_args share, set on ``a`` from the tuple ``_fused_inputs`` returns and
    ``flags`` (CAMERA_FLAGS; a member the struct lacks is skipped).  ``band`` = (b0, b1,
    rows, t_rand, pix_y): faces b0:b1 and ``rows`` image rows, with t_rand and pix_y already
    cut to them."""
    cam, focal, near, far, styles, t_rand, per_sample, pix_x, pix_y, t_vals = inputs
    if band is None:
        B = cam.shape[0]
    else:
        b0, b1, H, t_rand, pix_y = band
        B = b1 - b0
        cam, focal, near, far, styles = (t[b0:b1] for t in (cam, focal, near, far, styles))
    P = _lib.ptr
    a.B, a.H, a.W, a.N = B, H, W, N
    a.cam, a.focal, a.near_, a.far_ = P(cam), P(focal), P(near), P(far)
    a.styles = P(styles)
    a.pix_x, a.pix_y, a.t_vals = P(pix_x), P(pix_y), P(t_vals)
    a.t_rand, a.t_rand_per_sample = P(t_rand), int(per_sample)
    for k in CAMERA_FLAGS:
        if hasattr(a, k):
            setattr(a, k, int(flags[k]))
    return a


def render_args(B, H, W, N, cam, focal, near, far, styles, pix_x, pix_y, t_vals, t_rand,
                sigma_noise, flags: dict, rgb, features, sdf, xyz, mask, ws, prepacked):
    """sdfr_ngp_render_args (shared by the three networks' entry points)."""
    P = _lib.ptr
    a = camera_args(_lib.NgpRenderArgs(),
                    (cam, focal, near, far, styles, t_rand, flags["t_rand_per_sample"], pix_x,
                     pix_y, t_vals), H, W, N, flags)
    a.sigma_noise = P(sigma_noise)
    a.with_sdf = int(flags["with_sdf"])
    a.rgb, a.features, a.sdf = P(rgb), P(features), P(sdf)
    a.xyz, a.mask = P(xyz), P(mask)
    a.workspace, a.workspace_bytes = P(ws), ws.numel()
    a.field_precision = int(flags["field_precision"])
    a.max_field_segments = int(flags["max_field_segments"])
    a.prepacked = P(prepacked)
    return a


def workspace_bytes(kind: int, B: int, H: int, W: int, N: int, num_levels: int) -> int:
    """sdfr_render_{ngp,siren,fc}_workspace_bytes: each takes the sizes its workspace
    depends on, a prefix of (B, H, W, N, levels)."""
    fn = getattr(_lib.lib(), f"sdfr_render_{_lib.NETWORKS[kind].name}_workspace_bytes")
    return fn(*(B, H, W, N, num_levels)[:len(fn.argtypes)])


def render_forward(kind, w, a, stream):
    """sdfr_render_{ngp,siren,fc}_forward."""
    name = f"sdfr_render_{_lib.NETWORKS[kind].name}_forward"
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(w), ctypes.byref(a), stream), name)


from . import ops  # noqa: E402  (ops.py imports the functions above for sdfr::render_fused)


class FusedCalls:
    """The fused HIP path of ``VolumeFeatureRenderer``.  It reads the renderer's options
    and ``self.network`` and keeps no state but the two packing caches, ``_pack_cache``
    and ``_grad_pack_cache`` (``_prepacked``)."""

    def _net_kind(self):
        """0 ngp, 1 siren, 2 fc (the index into _lib.NETWORKS), None: no fused kernel."""
        return getattr(self.network, "net_kind", None)

    def _fused_inputs_ok(self, x, styles, no_grad_on=()):
        """What every fused call needs (the network's kind is the caller's to check first):
        ``use_fused``, ``x`` on the GPU, styles [B,256] for a 256-wide network, and under
        grad mode nothing that requires grad among styles, ``no_grad_on``, parameters."""
        if not self.use_fused or not x.is_cuda or styles is None:
            return False
        if styles.dim() != 2 or styles.shape[1] != 256 or self.network.W != 256:
            return False
        if torch.is_grad_enabled() and (styles.requires_grad or any(
                t.requires_grad for t in (*no_grad_on, *self.parameters()))):
            return False
        return True

    def _fused_ok(self, cam_poses, styles, return_eikonal):
        kind = self._net_kind()
        if kind is None or return_eikonal:
            return False
        if kind and (self.field_precision != "f16x3" or self.network.D != 8 or
                     len(self.network.pts_linears) != (8 if kind == 1 else 7)):
            return False
        return self._fused_inputs_ok(cam_poses, styles)

    def _query_fused_ok(self, points, styles):
        """The rule of ``_fused_ok`` for a point query (the fused query and gradient exist
        for the three networks on the f16x3 field kernel; SIREN and FC in the shape their
        kernels are built for: D = 8, W = 256)."""
        kind = self._net_kind()
        if kind is None or self.field_precision != "f16x3":
            return False
        if kind and (self.network.D != 8 or
                     len(self.network.pts_linears) != (8 if kind == 1 else 7)):
            return False
        return self._fused_inputs_ok(points, styles, no_grad_on=(points,))

    def _weight_tensors(self, kind):
        """The network's tensors in the order of ``_lib.NETWORKS[kind].fields``: the
        argument list of sdfr::render_fused, which weights_struct zips with the same tuple
        (sigmoid_beta is a placeholder without an SDF)."""
        net = self.network
        pts, views, sigma, rgb = list(net.pts_linears), net.views_linears, net.sigma_linear, \
            net.rgb_linear
        m = {"pts_w": [l.weight for l in pts], "pts_b": [l.bias for l in pts],
             "views_w": views.weight, "views_b": views.bias,
             "sigma_w": sigma.weight, "sigma_b": sigma.bias, "rgb_w": rgb.weight,
             "rgb_b": rgb.bias, "sigmoid_beta": self.sigmoid_beta if self.with_sdf else rgb.bias}
        if kind == 0:
            enc, inp = net.encoder, net.input_linear
            m.update(embeddings=enc.embeddings, offsets=enc.offsets, input_w=inp.weight,
                     input_b=inp.bias)
        if kind == 2:
            m.update(x_in_w=net.x_in.weight, x_in_b=net.x_in.bias,
                     style_w=net.style_in.weight, style_b=net.style_in.bias)
        else:
            gamma, beta = [l.gamma for l in (*pts, views)], [l.beta for l in (*pts, views)]
            m.update(pts_gw=[g.weight for g in gamma[:-1]], pts_gb=[g.bias for g in gamma[:-1]],
                     pts_bw=[b.weight for b in beta[:-1]], pts_bb=[b.bias for b in beta[:-1]],
                     views_gw=gamma[-1].weight, views_gb=gamma[-1].bias,
                     views_bw=beta[-1].weight, views_bb=beta[-1].bias)
        return [m[name] if i is None else m[name][i] for name, i in _SLOTS[kind]]

    def _weight_scalars(self, kind):
        """(fscal, iscal) of weights_struct."""
        net = self.network
        if kind == 0:
            return ([float(np.log2(net.encoder.per_level_scale)), float(net.bound)],
                    [int(net.encoder.base_resolution)])
        return [], [int(net.D), int(net.W)]

    def _weight_struct(self, kind):
        fs, is_ = self._weight_scalars(kind)
        return weights_struct(kind, self._weight_tensors(kind), fs, is_, self.with_sdf)

    def _fused_check_params(self):
        net, kind = self.network, self._net_kind()
        if kind == 2:
            if net.D != 8 or net.W != 256 or len(net.pts_linears) != 7:
                raise RuntimeError("fused fc renderer supports the SDFace FCGenerator "
                                   "(D=8, W=256) only")
        elif kind == 1:
            if net.D != 8 or net.W != 256 or net.input_ch_views != 3:
                raise RuntimeError("fused siren renderer supports the SDFace SirenGenerator "
                                   "(D=8, W=256) only")
        elif len(net.pts_linears) != 3 or net.encoder.num_levels != 16 or \
                net.encoder.level_dim != 2 or net.encoder_dir.degree != 4:
            raise RuntimeError("fused ngp renderer supports the SDFace NGPSIRENGenerator only")
        for p in self.parameters():
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise RuntimeError("fused ngp renderer needs contiguous fp32 parameters")

    def _fused_inputs(self, cam_poses, focal, near, far, styles, t_rand):
        """A camera call's inputs as the library takes them (contiguous fp32 on the cameras'
        device): ``cam, focal, near, far, styles, t_rand, per_sample, pix_x, pix_y, t_vals``.
        ``t_rand`` is None without ``perturb``, else [B,H,W] or (``per_sample`` = 1)
        [B,H,W,N], drawn here when none was given."""
        dev = cam_poses.device
        B = cam_poses.shape[0]
        cam = cam_poses.detach().float().contiguous()
        focal = _per_face(focal, B, dev)
        near = _per_face(near, B, dev)
        far = _per_face(far, B, dev)
        styles = styles.detach().float().contiguous()
        per_sample = 0
        if self.perturb > 0:
            shape = (B, self.out_im_res, self.out_im_res)
            if not self.offset_sampling:
                shape += (self.N_samples,)
                per_sample = 1
            if t_rand is None:
                t_rand = self._draw_t_rand(shape, dev)
            t_rand = t_rand.to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
        else:
            t_rand = None
        pix_x = self.i[0, 0, :].contiguous()
        pix_y = self.j[0, :, 0].contiguous()
        t_vals = self.t_vals.reshape(-1).contiguous()
        return cam, focal, near, far, styles, t_rand, per_sample, pix_x, pix_y, t_vals

    def _camera_flags(self):
        """CAMERA_FLAGS of camera_args, from the renderer's options."""
        return dict(
            offset_sampling=int(self.offset_sampling),
            static_viewdirs=int(bool(self.static_viewdirs)), z_normalize=int(self.z_normalize),
            force_background=int(bool(self.force_background)))

    def fused_forward(self, cam_poses, focal, near, far, styles, t_rand=None, encode_only=False,
                      styles_event=None, feat_mod=None):
        """The whole ngp render on libsdfr (no autograd).  Returns the same tuple
        as ``forward`` (rgb, features, sdf, mask, xyz, None).  ``styles_event``: a
        torch.cuda.Event after which ``styles`` is ready (computed on another
        stream): the library enqueues the sample geometry and the hash-grid gather
        before its wait on it (ABI 11).  ``feat_mod`` [B,256] (ngp / FC f16x3): the
        features come back as features * feat_mod in the decoder's split-NHWC fp16
        layout [B,H,W,32,2,8] (ABI 12; sdfr_modulate_to_nhwc_split's output, bit for bit)
        instead of NCHW fp32."""
        self._fused_check_params()
        dev = cam_poses.device
        if styles_event is not None and not (styles.dtype == torch.float32
                                             and styles.is_contiguous()):
            # a conversion would read the styles on this stream: wait here instead
            torch.cuda.current_stream(dev).wait_event(styles_event)
            styles_event = None
        B = cam_poses.shape[0]
        H = W = self.out_im_res
        N = self.N_samples
        cam, focal, near, far, styles, t_rand, per_sample, pix_x, pix_y, t_vals = \
            self._fused_inputs(cam_poses, focal, near, far, styles, t_rand)
        noise = None
        if not self.with_sdf and self.raw_noise_std > 0:
            noise = torch.randn(B, H, W, N, device=dev) * self.raw_noise_std
        kind = self._net_kind()
        if feat_mod is not None and (kind == 1 or self.field_precision != "f16x3"
                                     or not self.output_features):
            feat_mod = None                      # SIREN / fp32 field: NCHW features
        if self.field_precision not in ("f16x3", "fp32"):
            raise ValueError(f"field_precision must be 'f16x3' or 'fp32', "
                             f"got {self.field_precision!r}")
        if kind and encode_only:
            raise RuntimeError("only the ngp renderer has a hash-grid encode stage")
        flags = dict(
            self._camera_flags(), t_rand_per_sample=per_sample, with_sdf=int(self.with_sdf),
            field_precision=(_lib.FIELD_FP32 if self.field_precision == "fp32"
                             else _lib.FIELD_F16X3),
            max_field_segments=int(self.max_field_segments),
            output_features=int(bool(self.output_features)),
            return_sdf=int(bool(self.return_sdf)), return_xyz=int(bool(self.return_xyz)))
        prepacked = self._prepacked(kind, cam) if self.field_precision == "f16x3" else None
        if (styles_event is None and feat_mod is None and not encode_only
                and self.stage_events is None and self.field_event is None):
            # the plain call: the registered op (ops.py), outputs allocated there
            fs, is_ = self._weight_scalars(kind)
            out = torch.ops.sdfr.render_fused(
                kind, self._weight_tensors(kind), cam, focal, near, far, styles, t_rand, noise,
                pix_x, pix_y, t_vals, prepacked, fs, is_, [flags[k] for k in ops.RENDER_FLAGS],
                H, W, N)
            rgb, features, sdf, mask, xyz = map(ops._none_if_empty, out)
            return rgb, features, sdf, mask, xyz, None
        # with events (stage timing, the styles hand-off of Generator.forward), the
        # decoder-layout feature store or the encode stage alone: the library directly
        rgb, features, sdf, mask, xyz = ops._render_outputs(
            B, H, W, N, dev, self.output_features and feat_mod is None, self.return_sdf,
            self.return_xyz, torch.empty, absent_none=True)
        feat_split = (torch.empty(B, H, W, 32, 2, 8, device=dev, dtype=torch.float16)
                      if feat_mod is not None else None)
        num_levels = self.network.encoder.num_levels if kind == 0 else 0
        ws = torch.empty(workspace_bytes(kind, B, H, W, N, num_levels), dtype=torch.uint8,
                         device=dev)
        a = render_args(B, H, W, N, cam, focal, near, far, styles, pix_x, pix_y, t_vals,
                        t_rand, noise, flags, rgb, features, sdf, xyz, mask, ws, prepacked)
        if self.stage_events is not None:
            for k, ev in enumerate(self.stage_events):
                if ev is not None:               # (None: that point is not timed)
                    a.stage_events[k] = ctypes.c_void_p(ev.cuda_event)
        if self.field_event is not None:
            a.field_event = ctypes.c_void_p(self.field_event.cuda_event)
        if styles_event is not None:
            a.styles_event = ctypes.c_void_p(styles_event.cuda_event)
        if feat_split is not None:
            feat_mod = feat_mod.detach().float().contiguous()
            a.features_split, a.features_mod = _lib.ptr(feat_split), _lib.ptr(feat_mod)
            features = feat_split
        w = self._weight_struct(kind)
        if encode_only:
            _lib.check(_lib.lib().sdfr_render_ngp_encode_only(
                ctypes.byref(w), ctypes.byref(a), _lib.stream_of(cam)), "sdfr_render_ngp_encode_only")
            return ws
        render_forward(kind, w, a, _lib.stream_of(cam))
        return rgb, features, sdf, mask, xyz, None

    def _prepacked(self, kind, like, grad=False):
        """The field kernel's split-fp16 weight packing (row scales, scaled biases,
        MFMA fragments: sdfr_render_*_pack), redone only when a network parameter
        changed (data pointer or in-place version), not per call.  ``grad``: the SIREN
        gradient kernel's own packing of the SDF trunk (sdfr_query_siren_grad_pack), kept
        in a cache entry of its own beside the render's."""
        key = (kind,) + tuple((p.data_ptr(), p._version) for p in self.network.parameters())
        attr = "_grad_pack_cache" if grad else "_pack_cache"
        cache = getattr(self, attr, None)
        if cache is not None and cache[0] == key:
            return cache[1]
        L = _lib.lib()
        if grad:
            nbytes, name = L.sdfr_query_siren_grad_pack_bytes(), "sdfr_query_siren_grad_pack"
        else:
            nbytes = L.sdfr_render_pack_bytes(int(kind))
            name = f"sdfr_render_{_lib.NETWORKS[kind].name}_pack"
        buf = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
        w = self._weight_struct(kind)
        _lib.check(getattr(L, name)(ctypes.byref(w), _lib.ptr(buf), _lib.stream_of(like)), name)
        setattr(self, attr, (key, buf))
        return buf

    # ---------------------------------------------------------------- point query
    # Points per library call of the fused query.  The ngp workspace is about 144 bytes per
    # point (the 32 gathered features, the grid coordinate) plus 0.9 MB, so 2^20 points
    # bound it at ~152 MB; at 32 points per group that is 512 workgroups, two per CU.  (The
    # SIREN calls' workspace does not grow with the points; they share the chunking.)
    QUERY_CHUNK_POINTS = 1 << 20

    def _fused_query(self, points, dirs, styles, return_rgb=True, chunk_groups=None):
        """``sdfr_query_{ngp,siren,fc}_forward`` on grouped points:
        ``points`` [B,R,N,3], ``dirs`` [B,R,3] (one per group) -> (sdf [B,R,N],
        rgb [B,R,N,3] | None), in calls of at most ``chunk_groups`` groups per face."""
        self._fused_check_params()
        dev = points.device
        B, R, N = points.shape[:3]
        pts = points.detach().float().contiguous()
        styles = styles.detach().float().contiguous()
        sdf = torch.empty(B, R, N, device=dev)
        rgb = torch.empty(B, R, N, 3, device=dev) if return_rgb else None
        if chunk_groups is None:
            chunk_groups = max(16, self.QUERY_CHUNK_POINTS // (B * N) // 16 * 16)
        L = _lib.lib()
        kind = self._net_kind()
        prepacked = self._prepacked(kind, pts)
        w = self._weight_struct(kind)
        name = f"sdfr_query_{_lib.NETWORKS[kind].name}_forward"
        fn = getattr(L, name)
        ws_bytes = getattr(L, f"sdfr_query_{_lib.NETWORKS[kind].name}_workspace_bytes")

        def call(r, ins, outs, ws):
            a = _lib.QueryArgs(
                B=B, R=r, N=N, points=_lib.ptr(ins[0]), dirs=_lib.ptr(ins[1]),
                styles=_lib.ptr(styles), sdf=_lib.ptr(outs[0]), rgb=_lib.ptr(outs[1]),
                workspace=_lib.ptr(ws), workspace_bytes=ws.numel(),
                prepacked=_lib.ptr(prepacked))
            _lib.check(fn(ctypes.byref(w), ctypes.byref(a), _lib.stream_of(pts)), name)

        self._chunked_calls(R, chunk_groups, (pts, dirs.float()), (sdf, rgb),
                            lambda r: ws_bytes(B, r, N), call)
        return sdf, rgb

    @staticmethod
    def _chunked_calls(total, chunk, ins, outs, workspace_bytes, call):
        """``call(n, ins, outs, ws)`` on at most ``chunk`` of the ``total`` entries along
        dim 1 of the [B,total,..] tensors ``ins`` and ``outs`` (an output may be None) at a
        time.  A chunk is a call of its own on contiguous tensors: the caller's own when
        one chunk is the whole, else copies in and out.  The workspace grows to
        ``workspace_bytes(n)``; the last one is returned."""
        whole = total <= chunk
        ws = None
        for i0 in range(0, total, chunk):
            i1 = min(total, i0 + chunk)
            c_ins = [(t if whole else t[:, i0:i1]).contiguous() for t in ins]
            c_outs = [t if whole or t is None else
                      torch.empty((t.shape[0], i1 - i0) + t.shape[2:], device=t.device)
                      for t in outs]
            ws = _workspace(ws, workspace_bytes(i1 - i0), ins[0].device)
            call(i1 - i0, c_ins, c_outs, ws)
            if not whole:
                for t, c in zip(outs, c_outs):
                    if t is not None:
                        t[:, i0:i1] = c
        return ws

    # ---------------------------------------------------------------- SDF gradient
    # Points per library call of the fused gradient.  The workspace is 512 bytes per
    # point (the 32 gathered features and their 3 x 32 input derivatives) plus 0.9 MB, so
    # 2^18 points bound it at ~135 MB; at 32 points per workgroup pass that is 8192
    # passes over the call's 1024 workgroups.
    GRADIENT_CHUNK_POINTS = 1 << 18

    def _fused_gradient(self, points, styles, chunk_points=None, encode_only=False):
        """``sdfr_query_{ngp,siren,fc}_grad`` on ``points`` [B,M,3] in
        calls of at most ``chunk_points`` points per face."""
        self._fused_check_params()
        dev = points.device
        B, M = points.shape[:2]
        pts = points.detach().float().contiguous()
        styles = styles.detach().float().contiguous()
        sdf = torch.empty(B, M, device=dev)
        grad = torch.empty(B, M, 3, device=dev)
        if chunk_points is None:
            chunk_points = self.GRADIENT_CHUNK_POINTS // B
        chunk_points = max(32, int(chunk_points) // 32 * 32)
        if encode_only:
            chunk_points = max(chunk_points, M)      # one call: its workspace is the result
        L = _lib.lib()
        kind = self._net_kind()
        # (SIREN: the gradient kernel's own packing of the trunk, cached beside the render's;
        # ngp and FC: the render's packing)
        prepacked = self._prepacked(kind, pts, grad=kind == 1)
        w = self._weight_struct(kind)
        name = f"sdfr_query_{_lib.NETWORKS[kind].name}_grad"
        fn = getattr(L, name)
        ws_bytes = getattr(L, name + "_workspace_bytes")

        def call(m, ins, outs, ws):
            a = _lib.GradArgs(
                B=B, M=m, points=_lib.ptr(ins[0]), styles=_lib.ptr(styles),
                sdf=_lib.ptr(outs[0]), grad=_lib.ptr(outs[1]), workspace=_lib.ptr(ws),
                workspace_bytes=ws.numel(), prepacked=_lib.ptr(prepacked))
            _lib.check(fn(ctypes.byref(w), ctypes.byref(a), _lib.stream_of(pts)), name)

        ws = self._chunked_calls(M, chunk_points, (pts,), (sdf, grad),
                                 lambda m: ws_bytes(B, m), call)
        if encode_only:
            # the workspace starts with the gather's output [B][Mp][4][32], Mp = M up to 8
            Mp = (M + 7) // 8 * 8
            gd = ws[:B * Mp * 512].view(torch.float32).view(B, Mp, 4, 32)[:, :M]
            return gd[:, :, 0].clone(), gd[:, :, 1:].clone()
        return sdf, grad

    # ---------------------------------------------------------------- geometry and surface
    # Samples per library call of the fused surface render.  A bisection step evaluates only
    # H W points per face, a few workgroups' worth, so a call should hold as many faces as
    # it can: 2^22 samples take 32 faces of 64^2 x 24 or one of 128^2 x 128 in one call (four
    # calls of 2^20 samples took twice as long).  The ngp workspace is about 170 bytes per
    # sample, ~0.7 GB at this bound; the SIREN's about 25.
    SURFACE_CHUNK_POINTS = 1 << 22

    def _banded_calls(self, inputs, out, per_sample, chunk_points, max_faces, workspace_bytes,
                      call):
        """``call(band, dst, ws)`` once per band of a camera call's outputs ``out`` (name ->
        tensor; those named in ``per_sample`` are [B,H,W,N,..], the others NCHW maps): as
        many whole faces as ``chunk_points`` samples hold (at most ``max_faces``), or bands
        of whole rows of one face; a single row above the chunk is one call.  ``band`` is
        camera_args' (with t_rand and pix_y cut to it), ``dst`` the band of every output --
        a view where that is contiguous (the per-sample outputs), else a tensor of its own
        that is copied back -- and ``ws`` a workspace of ``workspace_bytes(faces, rows, W,
        N)`` bytes."""
        cam, t_rand, pix_y = inputs[0], inputs[5], inputs[8]
        dev, B = cam.device, cam.shape[0]
        H = W = self.out_im_res
        N = self.N_samples
        chunk_points = max(1, int(chunk_points))
        per_row, per_face = W * N, H * W * N
        if per_face <= chunk_points:
            faces, rows = max(1, min(chunk_points // per_face, max_faces)), H
        else:
            faces, rows = 1, max(1, chunk_points // per_row)
        ws = None
        for b0 in range(0, B, faces):
            b1 = min(B, b0 + faces)
            for y0 in range(0, H, rows):
                y1 = min(H, y0 + rows)
                dst, tmp = {}, {}
                for k, t in out.items():
                    v = t[b0:b1, y0:y1] if k in per_sample else t[b0:b1, :, y0:y1]
                    dst[k] = v if v.is_contiguous() else torch.empty(v.shape, device=dev,
                                                                     dtype=v.dtype)
                    if dst[k] is not v:
                        tmp[k] = v
                c_rand = None
                if t_rand is not None:
                    c_rand = t_rand[b0:b1, y0:y1].contiguous()
                ws = _workspace(ws, workspace_bytes(b1 - b0, y1 - y0, W, N), dev)
                call((b0, b1, y1 - y0, c_rand, pix_y[y0:y1]), dst, ws)
                for k, v in tmp.items():
                    v.copy_(dst[k])

    def _fused_geometry(self, cam_poses, focal, near, far, styles, t_rand, want, chunk_points):
        """``sdfr_render_ngp_geometry`` in calls of whole faces or bands of whole rows."""
        self._fused_check_params()
        dev = cam_poses.device
        B = cam_poses.shape[0]
        H = W = self.out_im_res
        N = self.N_samples
        inputs = self._fused_inputs(cam_poses, focal, near, far, styles, t_rand)
        shapes = {"sdf": (B, H, W, N), "eikonal": (B, H, W, N, 3), "normal": (B, 3, H, W),
                  "depth": (B, 1, H, W), "xyz": (B, 3, H, W), "mask": (B, 1, H, W)}
        out = {k: torch.empty(shapes[k], device=dev) for k in want}
        if chunk_points is None:
            chunk_points = self.GRADIENT_CHUNK_POINTS
        L = _lib.lib()
        flags = self._camera_flags()
        prepacked = self._prepacked(0, inputs[0])
        w = self._weight_struct(0)
        stream = _lib.stream_of(inputs[0])

        def call(band, dst, ws):
            a = _lib.NgpGeometryArgs(
                workspace=_lib.ptr(ws), workspace_bytes=ws.numel(),
                prepacked=_lib.ptr(prepacked),
                **{k: _lib.ptr(dst.get(k)) for k in self.GEOMETRY_FIELDS})
            camera_args(a, inputs, H, W, N, flags, band)
            _lib.check(L.sdfr_render_ngp_geometry(ctypes.byref(w), ctypes.byref(a), stream),
                       "sdfr_render_ngp_geometry")

        # the library takes fewer than 2^25 padded points per call
        self._banded_calls(inputs, out, ("sdf", "eikonal"), chunk_points,
                           ((1 << 25) - 1) // ((H * W * N + 7) // 8 * 8),
                           L.sdfr_render_ngp_geometry_workspace_bytes, call)
        if "sdf" in out:
            out["sdf"] = out["sdf"].unsqueeze(-1)
        return out

    def _fused_surface(self, cam_poses, focal, near, far, styles, t_rand, refine_steps, want,
                       chunk_points):
        """``sdfr_render_{ngp,siren}_surface`` in calls of whole faces or bands of rows."""
        self._fused_check_params()
        dev = cam_poses.device
        B = cam_poses.shape[0]
        H = W = self.out_im_res
        N = self.N_samples
        inputs = self._fused_inputs(cam_poses, focal, near, far, styles, t_rand)
        shapes = {k: (B, 3 if k in ("xyz", "normal", "rgb") else 1, H, W)
                  for k in self.SURFACE_FIELDS}
        shapes["sdf"] = (B, H, W, N)
        out = {k: torch.empty(shapes[k], device=dev,
                              dtype=torch.int32 if k == "sample" else torch.float32)
               for k in want}
        if chunk_points is None:
            chunk_points = self.SURFACE_CHUNK_POINTS
        L = _lib.lib()
        kind = self._net_kind()
        name = f"sdfr_render_{_lib.NETWORKS[kind].name}_surface"
        fn, ws_bytes = getattr(L, name), getattr(L, name + "_workspace_bytes")
        flags = self._camera_flags()
        prepacked = self._prepacked(kind, inputs[0])
        needs_grad = kind == 1 and ("normal" in want or "residual" in want)
        prepacked_grad = self._prepacked(kind, inputs[0], grad=True) if needs_grad else None
        w = self._weight_struct(kind)
        stream = _lib.stream_of(inputs[0])

        def need(*sizes):
            n = ws_bytes(*sizes)
            if n == 0:
                raise ValueError("render_surface: too many points in one call; lower "
                                 "chunk_points")
            return n

        def call(band, dst, ws):
            a = _lib.SurfaceArgs(
                refine_steps=refine_steps, workspace=_lib.ptr(ws), workspace_bytes=ws.numel(),
                prepacked=_lib.ptr(prepacked), prepacked_grad=_lib.ptr(prepacked_grad),
                **{k: _lib.ptr(dst.get(k)) for k in self.SURFACE_FIELDS})
            camera_args(a, inputs, H, W, N, flags, band)
            _lib.check(fn(ctypes.byref(w), ctypes.byref(a), stream), name)

        self._banded_calls(inputs, out, ("sdf",), chunk_points, B, need, call)
        if "sdf" in out:
            out["sdf"] = out["sdf"].unsqueeze(-1)
        return out

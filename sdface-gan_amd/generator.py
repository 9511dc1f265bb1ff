"""Generator (mapping + fused renderer + StyleGAN2 decoder), drop-in API.

Follows im2scene/sdf/models/sdf_model.py:
  MappingLinear :437-466   Upsample/Blur :480-538    EqualLinear :579-611
  ModulatedConv2d :614-701 NoiseInjection :704-792   StyledConv :795-818
  ToRGB :821-843           Decoder :883-1056         Generator :1059-1216
and the device-agnostic forms of the fused ops of sdf_op.py:105-120 / 259-314.

The decoder's modulated convolution runs as ``conv(x * s, W) * demod`` -- one
batched convolution instead of the reference's per-face grouped convolution
(same algebra, fp32); on the module path that convolution is MIOpen's.  On the
GPU, the bias/leaky-ReLU and upfirdn2d ops are the HIP kernels of
decoder_ops.py; at inference (no grad) the convolutions are the split-fp16
MFMA kernels of csrc/conv_f16x3.hip and everything between two of them is one
HIP epilogue, inside the conv kernel where it can be (decoder_fused.py:
``FusedDecoder``, which ``Decoder`` inherits).

Geometry-aware noise projection (``Generator.forward(project_noise=True, mesh_path=...)``
on a model built with ``project_noise``; the reference rasterises with pytorch3d) runs on
the HIP rasteriser of raster.py: ``NoiseInjection.project_noise`` gives every vertex of the
identity's mesh one N(0,1) value, rasterises the mesh from the frame's camera at the
layer's resolution and writes the interpolated values over the layer's fixed noise map
where the mesh covers a pixel, so the noise follows the surface through a camera sweep.
The ``Decoder`` forms those maps up front (one rasterisation per resolution) and then runs
its fused path.  Deliberate differences from the reference: the pose itself and the call's
focal length (scaled to the layer's resolution) are the camera, where the reference
rebuilds one from Euler angles at distance 1 and fov 12 degrees (``focal=None`` keeps that
fov); the nearest face's value, where pytorch3d blends the nearest faces softly; and B >= 1
views of the one mesh, where the reference asserts B = 1.
"""
from __future__ import annotations

import math
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from .decoder_fused import FusedDecoder
from .decoder_ops import FusedLeakyReLU, fused_leaky_relu, upfirdn2d  # noqa: F401
from .renderer import VolumeFeatureRenderer


def make_kernel(k):
    k = torch.tensor(k, dtype=torch.float32)
    if k.ndim == 1:
        k = k[None, :] * k[:, None]
    return k / k.sum()


class Upsample(nn.Module):
    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer("kernel", make_kernel(kernel) * (factor ** 2))
        p = self.kernel.shape[0] - factor
        self.pad = ((p + 1) // 2 + factor - 1, p // 2)

    def forward(self, input):
        return upfirdn2d(input, self.kernel, up=self.factor, down=1, pad=self.pad)


class Blur(nn.Module):
    def __init__(self, kernel, pad, upsample_factor=1):
        super().__init__()
        k = make_kernel(kernel)
        if upsample_factor > 1:
            k = k * (upsample_factor ** 2)
        self.register_buffer("kernel", k)
        self.pad = pad

    def forward(self, input):
        return upfirdn2d(input, self.kernel, pad=self.pad)


class PixelNorm(nn.Module):
    def forward(self, input):
        return input * torch.rsqrt(torch.mean(input ** 2, dim=1, keepdim=True) + 1e-8)


class MappingLinear(nn.Module):
    """Renderer mapping layer (sdf_model.py:437-466)."""

    def __init__(self, in_dim, out_dim, bias=True, activation=None, is_last=False):
        super().__init__()
        std = 0.25 if is_last else 1
        self.weight = nn.Parameter(std * nn.init.kaiming_normal_(
            torch.empty(out_dim, in_dim), a=0.2, mode="fan_in", nonlinearity="leaky_relu"))
        if bias:
            lim = math.sqrt(1 / in_dim)
            self.bias = nn.Parameter(nn.init.uniform_(torch.empty(out_dim), a=-lim, b=lim))
        else:
            self.bias = None
        self.activation = activation

    def forward(self, input):
        if self.activation is not None:
            return fused_leaky_relu(F.linear(input, self.weight), self.bias, scale=1)
        return F.linear(input, self.weight, bias=self.bias)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.weight.shape[1]}, {self.weight.shape[0]})"


class EqualLinear(nn.Module):
    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, lr_mul=1, activation=None):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_dim, in_dim).div_(lr_mul))
        self.bias = nn.Parameter(torch.zeros(out_dim).fill_(bias_init)) if bias else None
        self.activation = activation
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul
        self.lr_mul = lr_mul

    def forward(self, input):
        if self.activation:
            return fused_leaky_relu(F.linear(input, self.weight * self.scale),
                                    self.bias * self.lr_mul)
        return F.linear(input, self.weight * self.scale, bias=self.bias * self.lr_mul)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.weight.shape[1]}, {self.weight.shape[0]})"


def mapping_forward(seq, x):
    """A mapping network (nn.Sequential of PixelNorm / EqualLinear / MappingLinear) on
    the inference path: one HIP launch per linear layer (``sdfr_mapping_linear``,
    PixelNorm folded into the next layer) when ``x`` is on the GPU and no gradient
    is recorded; the modules themselves otherwise.  Same per-element arithmetic
    (W * scale, b * lr_mul, x + b, leaky ReLU, * scale); the dot products are
    summed in a different order than the GEMM's (fp32 rounding level)."""
    if not (x.is_cuda and not torch.is_grad_enabled() and x.dtype == torch.float32
            and x.dim() == 2):
        return seq(x)
    from . import _lib
    L = _lib.lib()
    pixelnorm = 0
    for m in seq:
        if isinstance(m, PixelNorm):
            pixelnorm = 1
            continue
        if isinstance(m, EqualLinear):
            wscale, bscale, act_scale = m.scale, m.lr_mul, 2 ** 0.5
        elif isinstance(m, MappingLinear):
            wscale, bscale, act_scale = 1.0, 1.0, 1.0
        else:
            return seq(x)                          # unknown layer: module path
        w = m.weight.detach()
        if w.shape[1] not in (256, 512) or not w.is_contiguous():
            return seq(x)
        x = x.contiguous()
        out = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.float32)
        _lib.check(L.sdfr_mapping_linear(
            _lib.ptr(out), _lib.ptr(x), _lib.ptr(w),
            _lib.ptr(m.bias.detach()) if m.bias is not None else None, x.shape[0], w.shape[1],
            w.shape[0], float(wscale), float(bscale), int(m.activation is not None), 0.2,
            float(act_scale), pixelnorm, _lib.stream_of(x)), "sdfr_mapping_linear")
        x, pixelnorm = out, 0
    if pixelnorm:
        return seq[-1](x)
    return x


class ModulatedConv2d(nn.Module):
    def __init__(self, in_channel, out_channel, kernel_size, style_dim, demodulate=True,
                 upsample=False, downsample=False, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        self.eps = 1e-8
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.upsample = upsample
        self.downsample = downsample
        if upsample:
            factor = 2
            p = (len(blur_kernel) - factor) - (kernel_size - 1)
            self.blur = Blur(blur_kernel, pad=((p + 1) // 2 + factor - 1, p // 2 + 1),
                             upsample_factor=factor)
        if downsample:
            factor = 2
            p = (len(blur_kernel) - factor) + (kernel_size - 1)
            self.blur = Blur(blur_kernel, pad=((p + 1) // 2, p // 2))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.padding = kernel_size // 2
        self.weight = nn.Parameter(torch.randn(1, out_channel, in_channel, kernel_size,
                                               kernel_size))
        self.modulation = EqualLinear(style_dim, in_channel, bias_init=1)
        self.demodulate = demodulate

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.in_channel}, {self.out_channel}, "
                f"{self.kernel_size}, upsample={self.upsample}, downsample={self.downsample})")

    def forward(self, input, style):
        batch = input.shape[0]
        s = self.modulation(style)                                   # [B, in]
        w = self.scale * self.weight[0]                              # [out, in, k, k]
        x = input * s.view(batch, -1, 1, 1)
        if self.upsample:
            out = F.conv_transpose2d(x, w.transpose(0, 1), padding=0, stride=2)
        elif self.downsample:
            out = F.conv2d(self.blur(x), w, padding=0, stride=2)
        else:
            out = F.conv2d(x, w, padding=self.padding)
        if self.demodulate:
            wsq = (w * w).sum([2, 3])                                # [out, in]
            demod = torch.rsqrt((s * s) @ wsq.t() + 1e-8)            # [B, out]
            out = out * demod.view(batch, -1, 1, 1)
        if self.upsample:
            out = self.blur(out)
        return out


class ProjectionCache:
    """What the noise-projecting layers of one ``Decoder`` share: the loaded meshes (one per
    (path, modification time) or ``Mesh`` object, with their subdivisions) and, during one
    ``Decoder.forward``, the rasterisation of each distinct (resolution, focal).  A plain
    object (not a module): every ``NoiseInjection`` of the decoder refers to the same one."""

    def __init__(self):
        self.meshes = {}
        self.rasters = None          # a dict only while a Decoder.forward is running

    def clear(self):
        self.meshes.clear()
        self.rasters = None

    def mesh(self, mesh_path, times):
        """``mesh_path`` (an .obj path or a ``Mesh``) subdivided ``times`` times."""
        from .mesh import Mesh
        from .raster import load_obj, subdivide_mesh
        if isinstance(mesh_path, Mesh):
            key = ("mesh", id(mesh_path))
            base = mesh_path
        else:
            import os
            path = os.fspath(mesh_path)
            key = ("path", path, os.stat(path).st_mtime_ns)
            base = None
        entry = self.meshes.get(key)
        if entry is None:
            # (one identity at a time: a sweep uses one mesh; an older one is dropped)
            self.meshes.clear()
            entry = self.meshes[key] = {0: base if base is not None else load_obj(path)}
        if times not in entry:
            prev = max(t for t in entry if t < times)
            entry[times] = subdivide_mesh(entry[prev], times - prev)
        return entry[times]


class NoiseInjection(nn.Module):
    """``image + weight * noise`` (sdf_model.py:704-792).  Built with ``project=True`` and
    given a noise map, a camera ``transform`` and a ``mesh_path``, the map is first
    projected through the mesh (``project_noise``)."""

    def __init__(self, project=False):
        super().__init__()
        self.project = project
        self.weight = nn.Parameter(torch.zeros(1))
        self.prev_noise = None
        self.mesh_fn = None
        self.vert_noise = None
        self._vert_noise_dev = None
        self.shared = ProjectionCache()     # a Decoder replaces it with its own
        # the image resolution that forward's ``focal`` refers to (None: this layer's own);
        # a Decoder sets its input resolution, the renderer's out_im_res
        self.focal_res = None

    @staticmethod
    def subdivisions(res):
        """The reference's rule (load_mc_mesh, sdf_model.py:728-752): the mesh as loaded up
        to 128^2, subdivided once at 256^2 and three times above."""
        return 0 if res <= 128 else (1 if res == 256 else 3)

    def reset_projected_noise(self):
        self.prev_noise = self.vert_noise = self._vert_noise_dev = self.mesh_fn = None

    def project_noise(self, noise, transform, mesh_path, focal=None, _key=None):
        """``noise`` [1 or B,1,r,r] with the identity's mesh drawn over it: every vertex of
        the mesh carries one N(0,1) value (``vert_noise`` [V,1], drawn once on the CPU with
        ``torch.empty(V, 1).normal_()`` and redrawn only when V changes), the mesh is
        rasterised from the B cameras ``transform`` [B,3,4] at r x r, and the result is
        ``where(covered, interpolated vert_noise, prev_noise)`` [B,1,r,r] -- ``prev_noise``
        being the first map this layer was ever given (it stays the background of every
        later call, as in the reference, until ``reset_projected_noise``).  So the noise
        sticks to the surface instead of the screen.  ``mesh_path``: an .obj path or a
        ``Mesh``; subdivided by ``subdivisions(r)``.  ``focal``: [B], [B,1,1] or a number in
        pixels of the r x r image; ``None`` is the reference's 12 degree field of view,
        (r / 2) / tan(6 degrees).

        Differences from the reference (sdf_model.py:754-782), on purpose: the mesh is
        projected with the pose itself (the reference rebuilds a camera from the pose's
        Euler angles at distance 1), so the noise lands on the pixels whose rays hit that
        surface point; the nearest face's value is used, not pytorch3d's soft blend of the
        nearest faces; B >= 1 views of the one mesh are allowed.  Needs the GPU: one
        ``sdfr_mesh_raster`` per distinct (r, focal) of a decoder call and one
        ``sdfr_mesh_interpolate`` per layer."""
        from .raster import (default_projection_focal, interpolate_vertex_attributes,
                             rasterize_mesh)
        if mesh_path is None or transform is None:
            raise ValueError("project_noise: needs the camera transform and a mesh_path")
        r = noise.shape[-1]
        if noise.shape[-2] != r:
            raise ValueError(f"project_noise: square noise maps only, got {tuple(noise.shape)}")
        if not noise.is_cuda:
            raise RuntimeError("project_noise: needs the GPU (HIP kernel)")
        self.mesh_fn = mesh_path
        mesh = self.shared.mesh(mesh_path, self.subdivisions(r))
        V = mesh.vertices.shape[0]
        if self.vert_noise is None or self.vert_noise.shape[0] != V:
            self.vert_noise = torch.empty(V, 1).normal_()
            self._vert_noise_dev = None
        if self._vert_noise_dev is None or self._vert_noise_dev.device != noise.device:
            self._vert_noise_dev = self.vert_noise.to(noise.device)
        if self.prev_noise is None:
            self.prev_noise = noise
        if focal is None:
            focal = default_projection_focal(r)
        # one rasterisation per resolution of a decoder call (``_key``: forward's, which
        # names the call's own focal and transform; the decoder holds both while it runs)
        rasters = self.shared.rasters if _key is not None else None
        raster = rasters.get(_key) if rasters is not None else None
        if raster is None:
            raster = rasterize_mesh(mesh, transform, focal, r)
            if rasters is not None:
                rasters[_key] = raster
        return interpolate_vertex_attributes(mesh, raster, self._vert_noise_dev,
                                             background=self.prev_noise.to(noise.device))

    def forward(self, image, noise=None, transform=None, mesh_path=None, focal=None):
        batch, _, height, width = image.shape
        if noise is None:
            noise = image.new_empty(batch, 1, height, width).normal_()
        elif self.project and transform is not None:
            key = (height, id(focal), id(transform))
            if focal is not None and self.focal_res is not None:
                focal = focal * (height / self.focal_res)
            noise = self.project_noise(noise, transform, mesh_path, focal, _key=key)
        return image + self.weight * noise


class StyledConv(nn.Module):
    def __init__(self, in_channel, out_channel, kernel_size, style_dim, upsample=False,
                 blur_kernel=(1, 3, 3, 1), project_noise=False):
        super().__init__()
        self.conv = ModulatedConv2d(in_channel, out_channel, kernel_size, style_dim,
                                    upsample=upsample, blur_kernel=blur_kernel)
        self.noise = NoiseInjection(project=project_noise)
        self.bias = nn.Parameter(torch.zeros(1, out_channel, 1, 1))
        self.activate = FusedLeakyReLU(out_channel)

    def forward(self, input, style, noise=None, transform=None, mesh_path=None, focal=None):
        out = self.conv(input, style)
        out = self.noise(out, noise=noise, transform=transform, mesh_path=mesh_path,
                         focal=focal)
        return self.activate(out)


class ToRGB(nn.Module):
    def __init__(self, in_channel, style_dim, upsample=True, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        self.upsample = Upsample(blur_kernel) if upsample else upsample
        self.conv = ModulatedConv2d(in_channel, 3, 1, style_dim, demodulate=False)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))

    def forward(self, input, style, skip=None):
        out = self.conv(input, style) + self.bias
        if skip is not None:
            if self.upsample:
                skip = self.upsample(skip)
            out = out + skip
        return out


class Decoder(FusedDecoder, nn.Module):
    """StyleGAN2 2D decoder, 64^2 x 256 features -> size^2 RGB (sdf_model.py:883-1056).
    Its fused inference path (``fused_ready``, ``prepare_fused``, ``_fused_forward``) is
    decoder_fused.FusedDecoder."""

    def __init__(self, model_opt, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        o = model_opt
        self.size = o.size
        self.style_dim = o.style_dim * 2
        in_dim = self.style_dim if o.psp else self.style_dim // 2
        layers = [PixelNorm(), EqualLinear(in_dim, self.style_dim, lr_mul=o.lr_mapping,
                                           activation="fused_lrelu")]
        for _ in range(4):
            layers.append(EqualLinear(self.style_dim, self.style_dim, lr_mul=o.lr_mapping,
                                      activation="fused_lrelu"))
        self.style = nn.Sequential(*layers)
        cm = o.channel_multiplier
        self.channels = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm,
                         256: 64 * cm, 512: 32 * cm, 1024: 16 * cm}
        dec_in = o.renderer_spatial_output_dim
        self.log_size = int(math.log(self.size, 2))
        self.log_in_size = int(math.log(dec_in, 2))
        in_feat = o.feature_encoder_in_channels if not o.psp else self.style_dim
        self.conv1 = StyledConv(in_feat, self.channels[dec_in], 3, self.style_dim,
                                blur_kernel=blur_kernel, project_noise=o.project_noise)
        self.to_rgb1 = ToRGB(self.channels[dec_in], self.style_dim, upsample=False)
        self.num_layers = (self.log_size - self.log_in_size) * 2 + 1
        self.convs = nn.ModuleList()
        self.upsamples = nn.ModuleList()
        self.to_rgbs = nn.ModuleList()
        self.noises = nn.Module()
        in_ch = self.channels[dec_in]
        for idx in range(self.num_layers):
            res = (idx + 2 * self.log_in_size + 1) // 2
            self.noises.register_buffer(f"noise_{idx}", torch.randn(1, 1, 2 ** res, 2 ** res))
        for i in range(self.log_in_size + 1, self.log_size + 1):
            out_ch = self.channels[2 ** i]
            self.convs.append(StyledConv(in_ch, out_ch, 3, self.style_dim, upsample=True,
                                         blur_kernel=blur_kernel,
                                         project_noise=o.project_noise))
            self.convs.append(StyledConv(out_ch, out_ch, 3, self.style_dim,
                                         blur_kernel=blur_kernel,
                                         project_noise=o.project_noise))
            self.to_rgbs.append(ToRGB(out_ch, self.style_dim))
            in_ch = out_ch
        self.n_latent = (self.log_size - self.log_in_size) * 2 + 2
        # noise projection (project_noise): the layers share one mesh cache and, within a
        # forward, one rasterisation per resolution; forward's focal is in pixels of the
        # decoder's input (the renderer's out_im_res)
        self._proj = ProjectionCache()
        for sc in [self.conv1] + list(self.convs):
            sc.noise.shared = self._proj
            sc.noise.focal_res = dec_in
        self.use_fused = True      # HIP epilogues on the inference path (GPU, no grad)
        # convolutions of the fused path: "f16x3" (split-fp16 MFMA implicit GEMM,
        # csrc/conv_f16x3.hip) or "miopen" (F.conv2d / conv_transpose2d, fp32)
        self.conv_impl = "f16x3"
        # regular f16x3 convs with the styled epilogue fused into the conv kernel
        # (sdfr_conv3x3_f16x3_act + sdfr_rgb_finish) instead of a separate pass
        self.fuse_conv_act = True
        # upsampling convs with the blur + styled epilogue inside conv_t_kernel
        # (sdfr_conv_t_act) wherever that kernel runs (>= 256 tiles: batches of 4+)
        self.fuse_conv_t_blur = True
        # profiling: (start, end) HIP event pairs recorded on the current stream around
        # the fused regular convolutions (conv_h_kernel) of the next forward, in order,
        # and their fp32-equivalent FLOPs (bench.py's decoder roofline)
        self.conv_events = None
        self.conv_flops = 0
        self._conv_ev = 0
        self._plan = None          # decoder_fused.DecoderPlan of the current weights

    def mean_latent(self, renderer_latent):
        return self.style(renderer_latent).mean(0, keepdim=True)

    def get_latent(self, input):
        return self.style(input)

    def styles_and_noise_forward(self, styles, noise, inject_index=None, truncation=1,
                                 truncation_latent=None, input_is_latent=False,
                                 randomize_noise=True):
        if not input_is_latent:
            styles = [mapping_forward(self.style, s) for s in styles]
        if noise is None:
            noise = ([None] * self.num_layers if randomize_noise else
                     [getattr(self.noises, f"noise_{i}") for i in range(self.num_layers)])
        if truncation < 1:
            styles = [truncation_latent[1] + truncation * (s - truncation_latent[1])
                      for s in styles]
        if len(styles) < 2:
            inject_index = self.n_latent
            latent = (styles[0].unsqueeze(1).repeat(1, inject_index, 1)
                      if styles[0].ndim < 3 else styles[0])
        else:
            if inject_index is None:
                inject_index = random.randint(1, self.n_latent - 1)
            latent = torch.cat([styles[0].unsqueeze(1).repeat(1, inject_index, 1),
                                styles[1].unsqueeze(1).repeat(1, self.n_latent - inject_index, 1)],
                               1)
        return latent, noise

    def reset_projected_noise(self):
        """Forget what noise projection keeps between calls: every layer's background map
        (``prev_noise``) and per-vertex noise (``vert_noise``), and the loaded meshes."""
        for sc in [self.conv1] + list(self.convs):
            sc.noise.reset_projected_noise()
        self._proj.clear()

    def _projects(self, transform):
        return transform is not None and self.conv1.noise.project

    def _projected_noise(self, noise, transform, mesh_path, focal):
        """The noise maps of a projected call, layer by layer in the module path's order
        (each layer's ``NoiseInjection.forward`` arithmetic on the map alone): [B,1,r,r]
        where a map was given, ``None`` (fresh noise) where not."""
        out = []
        for sc, n in zip([self.conv1] + list(self.convs), noise):
            if n is not None:
                r = n.shape[-1]
                key = (r, id(focal), id(transform))
                f = focal if focal is None else focal * (r / sc.noise.focal_res)
                n = sc.noise.project_noise(n, transform, mesh_path, f, _key=key)
            out.append(n)
        return out

    def forward(self, features, styles, rgbd_in=None, transform=None, return_latents=False,
                inject_index=None, truncation=1, truncation_latent=None, input_is_latent=False,
                noise=None, randomize_noise=True, mesh_path=None, prepared=None, focal=None):
        # projected noise: the maps are formed up front (one rasterisation per
        # resolution, shared by its layers while this call runs), and the decoder then
        # runs as it does without a transform -- through the fused path where that applies
        projects = self._projects(transform)
        if projects and mesh_path is None:
            raise ValueError("Decoder: project_noise needs a mesh_path")
        self._proj.rasters = {} if projects else None
        try:
            return self._forward(features, styles, rgbd_in, transform, return_latents,
                                 inject_index, truncation, truncation_latent, input_is_latent,
                                 noise, randomize_noise, mesh_path, prepared, focal)
        finally:
            self._proj.rasters = None

    def _forward(self, features, styles, rgbd_in, transform, return_latents, inject_index,
                 truncation, truncation_latent, input_is_latent, noise, randomize_noise,
                 mesh_path, prepared, focal):
        if prepared is not None:         # prepare_fused() ran earlier (Generator.forward)
            latent, noise, sty = prepared
            if self._fused_ok(features, rgbd_in, transform):
                return (self._fused_forward(features, latent, noise, sty),
                        (latent if return_latents else None))
            # the features turned out to need the autograd path (they require grad):
            # run the module path below on the prep's latent and noise maps -- drawing
            # them again would shift the RNG streams against the reference's order
        else:
            latent, noise = self.styles_and_noise_forward(styles, noise, inject_index,
                                                          truncation, truncation_latent,
                                                          input_is_latent, randomize_noise)
            if self._projects(transform) and self._fused_ok(features, rgbd_in, None):
                noise = self._projected_noise(noise, transform, mesh_path, focal)
                transform = None
            if self._fused_ok(features, rgbd_in, transform):
                return (self._fused_forward(features, latent, noise),
                        (latent if return_latents else None))
        out = self.conv1(features, latent[:, 0], noise=noise[0], transform=transform,
                         mesh_path=mesh_path, focal=focal)
        skip = self.to_rgb1(out, latent[:, 1], skip=rgbd_in)
        i = 1
        for c1, c2, n1, n2, to_rgb in zip(self.convs[::2], self.convs[1::2], noise[1::2],
                                          noise[2::2], self.to_rgbs):
            out = c1(out, latent[:, i], noise=n1, transform=transform, mesh_path=mesh_path,
                     focal=focal)
            out = c2(out, latent[:, i + 1], noise=n2, transform=transform, mesh_path=mesh_path,
                     focal=focal)
            skip = to_rgb(out, latent[:, i + 2], skip=skip)
            i += 2
        return skip, (latent if return_latents else None)


_SIDE_STREAMS = {}


def _tensors_of(x):
    """Every tensor inside nested tuples / lists / dicts (Decoder.prepare_fused's result:
    the demodulations are a dict of views of one flat buffer)."""
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, dict):
        for y in x.values():
            yield from _tensors_of(y)
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from _tensors_of(y)


def _has(o, k):
    return k in o.keys() if hasattr(o, "keys") else hasattr(o, k)


class Generator(nn.Module):
    """Drop-in for sdf_model.py:1059-1216."""

    def __init__(self, model_opt, renderer_opt, blur_kernel=(1, 3, 3, 1), ema=False,
                 full_pipeline=True):
        super().__init__()
        self.size = model_opt.size
        self.style_dim = model_opt.style_dim * 2 if model_opt.psp else model_opt.style_dim
        self.num_layers = 1
        self.train_renderer = not model_opt.freeze_renderer
        self.full_pipeline = full_pipeline
        model_opt.feature_encoder_in_channels = renderer_opt.width
        self.is_train = not (ema or _has(model_opt, "is_test"))
        self.style = nn.Sequential(*[MappingLinear(self.style_dim, self.style_dim,
                                                   activation="fused_lrelu") for _ in range(3)])
        self.renderer = VolumeFeatureRenderer(renderer_opt, style_dim=self.style_dim,
                                              out_im_res=model_opt.renderer_spatial_output_dim)
        if self.full_pipeline:
            self.decoder = Decoder(model_opt, blur_kernel=blur_kernel)
        # fused inference: decoder prep (its mapping network, noise, modulations and
        # demodulations) on a side stream beside the renderer.  Round 3 measured it
        # within noise (profiles/round3_overlap_ab.json: the gather beside it slowed
        # 0.774 -> 0.801 ms); since the prep's small kernels were shortened in round 5
        # it is +0.8 % at 32 faces (3251 -> 3278 faces/s, six interleaved samples each,
        # scripts/overlap_b32.py) and neutral at one face, so it is on by default
        self.overlap_decoder_prep = True
        # the field kernel stores the decoder's first input (features x modulation,
        # split-NHWC) instead of NCHW features for modulate_nhwc_kernel to convert
        self.fuse_feature_split = True
        self.feature_split_min_batch = 4
        # repeated plain inference calls (eval.py's loop) replay a HIP graph of the
        # whole forward, captured on the second sighting of the call (graphs.py,
        # ForwardGraphCache): same results and random streams as the eager path
        self.graph_inference = True
        self._dec_key = None

    def _decoder_weights_unchanged(self):
        """Is the decoder's plan key the one of the last time this was asked?  (Asked right
        after decoder.fused_ready(), which made the plan the current weights'.)"""
        key = self.decoder._plan.key
        same = key == self._dec_key
        self._dec_key = key
        return same

    @staticmethod
    def _side_stream(device):
        # one per device for the process (kept off the module: a Stream does not deepcopy)
        st = _SIDE_STREAMS.get(device)
        if st is None:
            st = _SIDE_STREAMS[device] = torch.cuda.Stream(device=device)
        return st

    def mean_latent(self, n_latent, device, z=None):
        if z is None:
            z = torch.randn(n_latent, self.style_dim, device=device)
        renderer_latent = self.style(z)
        renderer_latent_mean = renderer_latent.mean(0, keepdim=True)
        decoder_latent_mean = (self.decoder.mean_latent(renderer_latent)
                               if self.full_pipeline else None)
        return [renderer_latent_mean, decoder_latent_mean]

    def get_latent(self, input):
        return self.style(input)

    def styles_and_noise_forward(self, styles, inject_index=None, truncation=1,
                                 truncation_latent=None, input_is_latent=False):
        if not input_is_latent:
            styles = [mapping_forward(self.style, s) for s in styles]
        if truncation < 1:
            styles = [truncation_latent[0] + truncation * (s - truncation_latent[0])
                      for s in styles]
        return styles

    def init_forward(self, styles, cam_poses, focals, near=0.88, far=1.12, t_rand=None):
        latent = self.styles_and_noise_forward(styles)
        return self.renderer.mlp_init_pass(cam_poses, focals, near, far, styles=latent[0],
                                           t_rand=t_rand)

    def _renderer_latent(self, styles, truncation=1, truncation_latent=None,
                         input_is_latent=False):
        """The renderer's latent [B,256] of ``styles``: the mapping network and truncation
        of ``forward`` (``styles_and_noise_forward``)."""
        latent = self.styles_and_noise_forward(styles, None, truncation, truncation_latent,
                                               input_is_latent)
        return latent[0][:, 0] if input_is_latent else latent[0]

    def query_field(self, points, styles, viewdirs=None, truncation=1, truncation_latent=None,
                    input_is_latent=False, return_rgb=True):
        """The renderer's field at ``points`` [B,M,3] (network coordinates) for the faces
        of ``styles``: the mapping network and truncation of ``forward``
        (``styles_and_noise_forward``), then ``VolumeFeatureRenderer.query`` ->
        ``(sdf [B,M], rgb [B,M,3] | None)``."""
        lat0 = self._renderer_latent(styles, truncation, truncation_latent, input_is_latent)
        return self.renderer.query(points, lat0, viewdirs=viewdirs, return_rgb=return_rgb)

    def query_field_gradient(self, points, styles, truncation=1, truncation_latent=None,
                             input_is_latent=False, normalize=False, chunk_points=None):
        """The SDF and its gradient at ``points`` [B,M,3] (network coordinates) for the
        faces of ``styles``: the mapping network and truncation of ``query_field``, then
        ``VolumeFeatureRenderer.query_gradient`` -> ``(sdf [B,M], grad [B,M,3])``."""
        lat0 = self._renderer_latent(styles, truncation, truncation_latent, input_is_latent)
        return self.renderer.query_gradient(points, lat0, normalize=normalize,
                                            chunk_points=chunk_points)

    def extract_mesh(self, styles, res=512, truncation=1, truncation_latent=None,
                     input_is_latent=False, **kw):
        """The mesh of the face of ``styles`` (one face) from narrow-band bricks: the
        mapping network and truncation of ``query_field``, then ``mesh.extract_mesh_sparse``
        (``kw``: level, lipschitz, grow, return_volume, components -- e.g.
        ``components={"largest": 1}`` keeps the largest connected component -- and simplify:
        ``simplify=4`` clusters the vertices of 4^3 lattice cells on the GPU before the copy,
        and smooth: ``smooth=10`` runs 10 Taubin iterations of ``mesh.smooth_mesh`` on the GPU
        after that, or a dict of its keyword arguments) -> ``Mesh``."""
        from .mesh import extract_mesh_sparse
        lat0 = self._renderer_latent(styles, truncation, truncation_latent, input_is_latent)
        return extract_mesh_sparse(self.renderer, lat0, res=res, **kw)

    def render_geometry(self, styles, cam_poses, focals, near, far, truncation=1,
                        truncation_latent=None, input_is_latent=False, **kw):
        """The geometry of the faces of ``styles`` seen from ``cam_poses``: the mapping
        network and truncation of ``query_field_gradient``, then
        ``VolumeFeatureRenderer.render_geometry`` (``kw``: t_rand, want, normalize,
        chunk_points) -> ``Geometry``.  Not part of the forward graph cache."""
        lat0 = self._renderer_latent(styles, truncation, truncation_latent, input_is_latent)
        return self.renderer.render_geometry(cam_poses, focals, near, far, lat0, **kw)

    def render_surface(self, styles, cam_poses, focals, near, far, truncation=1,
                       truncation_latent=None, input_is_latent=False, **kw):
        """The surface of the faces of ``styles`` seen from ``cam_poses``: the mapping
        network and truncation of ``render_geometry``, then
        ``VolumeFeatureRenderer.render_surface`` (``kw``: t_rand, refine_steps, want,
        chunk_points) -> ``Surface``.  Not part of the forward graph cache."""
        lat0 = self._renderer_latent(styles, truncation, truncation_latent, input_is_latent)
        return self.renderer.render_surface(cam_poses, focals, near, far, lat0, **kw)

    def forward(self, styles, cam_poses, focals, near=0.88, far=1.12, return_latents=False,
                inject_index=None, truncation=1, truncation_latent=None, input_is_latent=False,
                noise=None, randomize_noise=True, return_sdf=False, return_xyz=False,
                return_eikonal=False, project_noise=False, mesh_path=None, t_rand=None):
        kw = dict(return_latents=return_latents, inject_index=inject_index,
                  truncation=truncation, truncation_latent=truncation_latent,
                  input_is_latent=input_is_latent, noise=noise, randomize_noise=randomize_noise,
                  return_sdf=return_sdf, return_xyz=return_xyz, return_eikonal=return_eikonal,
                  project_noise=project_noise, mesh_path=mesh_path, t_rand=t_rand)
        if self.graph_inference and not self.training and not torch.is_grad_enabled():
            from .graphs import forward_cache
            cache = forward_cache(self)
            if cache.eligible(self, styles, cam_poses, focals, near, far, kw):
                out = cache(self, styles, cam_poses, focals, near, far, kw)
                if out is not None:
                    return out
        return self._forward_eager(styles, cam_poses, focals, near, far, **kw)

    def _forward_eager(self, styles, cam_poses, focals, near=0.88, far=1.12,
                       return_latents=False, inject_index=None, truncation=1,
                       truncation_latent=None, input_is_latent=False, noise=None,
                       randomize_noise=True, return_sdf=False, return_xyz=False,
                       return_eikonal=False, project_noise=False, mesh_path=None, t_rand=None):
        grad_on = self.is_train and self.train_renderer
        # Fused inference: the decoder's feature-independent prep (its mapping network,
        # noise maps, per-layer modulations / demodulations: ~12 small launches) runs
        # before the renderer -- on a side stream beside it while the decoder's weight
        # caches are warm (weights unchanged since the previous call), else in order
        # on this stream, so the caches a weight update rebuilds, and the ones it
        # frees, never cross streams.  On the side stream the renderer's own mapping
        # network goes there too: the renderer enqueues its sample geometry and hash-grid
        # gather (which do not read the styles) ahead of its wait on `styles_ev` (ABI 11).
        # Either way the device RNG is drawn in the same order (decoder noise, then the
        # renderer's sampling offsets).
        prepared, side, styles_ev = None, None, None
        B, dev = cam_poses.shape[0], cam_poses.device
        kw = dict(noise=noise, inject_index=inject_index, truncation=truncation,
                  truncation_latent=truncation_latent, input_is_latent=input_is_latent,
                  randomize_noise=randomize_noise)
        # features needing grad (renderer trained, or latents requiring grad) take the
        # decoder's autograd path: no prep then (Decoder.forward re-checks as well)
        pre_grad = grad_on and (
            any(p.requires_grad for p in self.renderer.parameters())
            or any(p.requires_grad for p in self.style.parameters())
            or any(s.requires_grad for s in styles))
        capturing = cam_poses.is_cuda and torch.cuda.is_current_stream_capturing()
        # (a small eager batch is host-bound: the stream switch would cost more than
        # the overlap saves; inside a graph capture it costs nothing at replay)
        if (self.full_pipeline and cam_poses.is_cuda and not project_noise and not pre_grad
                and self.overlap_decoder_prep and (B >= 8 or capturing)
                and self.decoder.fused_ready(dev) and self._decoder_weights_unchanged()):
            main = torch.cuda.current_stream(dev)
            side = self._side_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                with torch.set_grad_enabled(grad_on):
                    latent = self.styles_and_noise_forward(styles, inject_index, truncation,
                                                           truncation_latent, input_is_latent)
                prepared = self.decoder.prepare_fused(latent, B, dev, **kw)
                # (after the prep: the field kernel also reads its first modulation)
                styles_ev = torch.cuda.Event()
                styles_ev.record(side)
            if not capturing:
                for t in list(_tensors_of(prepared)) + list(_tensors_of(latent)):
                    t.record_stream(main)            # made on `side`, used on `main`
        else:
            with torch.set_grad_enabled(grad_on):
                latent = self.styles_and_noise_forward(styles, inject_index, truncation,
                                                       truncation_latent, input_is_latent)
            render_grad = grad_on and (
                any(p.requires_grad for p in self.renderer.parameters())
                or any(s.requires_grad for s in latent))
            if (self.full_pipeline and cam_poses.is_cuda and not project_noise and not render_grad
                    and self.decoder.fused_ready(dev)):
                prepared = self.decoder.prepare_fused(latent, B, dev, **kw)
        # the fused decoder's first layer input (features x its modulation, split-NHWC)
        # straight from the field kernel's feature store (ABI 12): one streaming pass less
        # (from 4 faces: below that the field kernel splits rays into segments and the
        # merge kernel would scatter 2-B split stores instead of coalesced NCHW rows)
        feat_mod = None
        if (prepared is not None and self.fuse_feature_split
                and B >= self.feature_split_min_batch
                and self.decoder._plan.layers[0].split):
            feat_mod = prepared.styles.mods[0]
        with torch.set_grad_enabled(grad_on):
            lat0 = latent[0][:, 0] if input_is_latent else latent[0]
            thumb_rgb, features, sdf, mask, xyz, eikonal_term = self.renderer(
                cam_poses, focals, near, far, styles=lat0, return_eikonal=return_eikonal,
                t_rand=t_rand, styles_event=styles_ev, feat_mod=feat_mod)
        if self.full_pipeline:
            # (the side stream's work ends at styles_ev, which the renderer made this
            # stream wait on before its FiLM prep -- every render entry does, ABI 11 --
            # so the decoder needs no second join: one right here would sit behind the
            # field kernel as a barrier packet, ~10 us of idle GPU per call)
            rgb, decoder_latent = self.decoder(
                features, latent, transform=cam_poses if project_noise else None,
                return_latents=return_latents, inject_index=inject_index, truncation=truncation,
                truncation_latent=truncation_latent, noise=noise,
                input_is_latent=input_is_latent, randomize_noise=randomize_noise,
                mesh_path=mesh_path, prepared=prepared,
                focal=focals if project_noise else None)
        else:
            rgb = None
        if return_latents:
            return rgb, decoder_latent
        out = (rgb, thumb_rgb)
        if return_xyz:
            out += (xyz,)
        if return_sdf:
            out += (sdf,)
        if return_eikonal:
            out += (eikonal_term,)
        if return_xyz:
            out += (mask,)
        return out

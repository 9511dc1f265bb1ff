"""Volume renderer: drop-in VolumeFeatureRenderer + its networks, MI355X path.

Module / parameter names, constructor arguments, initialisation (including the
order in which the CPU RNG is consumed) and forward signatures follow
``im2scene/sdf/models/sdf_model.py``:

  LinearLayer          :23-41     FiLMSiren          :44-69
  SirenGenerator       :101-139   VolumeFeatureRenderer :143-423
  get_encoder          :1512-1531 NGPSIRENGenerator  :1534-1596
  FCGenerator          :1599-1670

``VolumeFeatureRenderer.forward`` runs the fused HIP renderer
(``sdfr_render_ngp_forward``: sampling + hash grid + MLP on MFMA + compositing)
whenever the network is the ngp one and no gradient is required (eval.py,
sdf_mesh.py, stage-2 training where the renderer is frozen).  When gradients
are needed (stage-1 training, eikonal term) it runs the reference's op-by-op
structure on the GPU, with the hash-grid and SH encoders on the HIP kernels.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.autograd as autograd
import torch.nn as nn
import torch.nn.functional as F

from .encoders import GridEncoder, SHEncoder
from .linear import film_linear, linear
from .render_calls import FusedCalls


# ---------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------
class LinearLayer(nn.Module):
    """SIREN linear layer: ``std_init * (x W^T + b) + bias_init`` (sdf_model.py:23-41)."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, std_init=1, freq_init=False,
                 is_first=False):
        super().__init__()
        if is_first:
            w = torch.empty(out_dim, in_dim).uniform_(-1 / in_dim, 1 / in_dim)
        elif freq_init:
            lim = np.sqrt(6 / in_dim) / 25
            w = torch.empty(out_dim, in_dim).uniform_(-lim, lim)
        else:
            w = 0.25 * nn.init.kaiming_normal_(torch.randn(out_dim, in_dim), a=0.2,
                                               mode="fan_in", nonlinearity="leaky_relu")
        self.weight = nn.Parameter(w)
        lim = np.sqrt(1 / in_dim)
        self.bias = nn.Parameter(nn.init.uniform_(torch.empty(out_dim), a=-lim, b=lim))
        self.bias_init = bias_init
        self.std_init = std_init

    # the renderer networks' layers take the training kernels (linear.py); others F.linear
    train_kernels = False
    double_backward = False       # set by SirenGenerator (its eikonal loss, linear.py)

    def forward(self, input):
        # linear(): F.linear, or the split-fp16 MFMA kernels for the renderer MLP's
        # training shapes (linear.py).  The reference's ``1 * y + 0`` (the defaults) is
        # the identity up to the sign of zero; skipping it saves two full passes over
        # the [rays, samples, 256] activation forward and one backward.
        y = linear(input, self.weight, self.bias, self.train_kernels, self.double_backward)
        if self.std_init != 1:
            y = self.std_init * y
        if self.bias_init != 0:
            y = y + self.bias_init
        return y


class FiLMSiren(nn.Module):
    """``sin(gamma(style) * (x W^T + b) + beta(style))`` (sdf_model.py:44-69)."""

    train_kernels = False         # set by NGPSIRENGenerator / SirenGenerator (linear.py)
    double_backward = False       # set by SirenGenerator (its eikonal loss, linear.py)

    def __init__(self, in_channel, out_channel, style_dim, is_first=False):
        super().__init__()
        self.in_channel = in_channel
        self.out_channel = out_channel
        if is_first:
            w = torch.empty(out_channel, in_channel).uniform_(-1 / 3, 1 / 3)
        else:
            lim = np.sqrt(6 / in_channel) / 25
            w = torch.empty(out_channel, in_channel).uniform_(-lim, lim)
        self.weight = nn.Parameter(w)
        lim = np.sqrt(1 / in_channel)
        self.bias = nn.Parameter(nn.init.uniform_(torch.empty(out_channel), a=-lim, b=lim))
        self.activation = torch.sin
        self.gamma = LinearLayer(style_dim, out_channel, bias_init=30, std_init=15)
        self.beta = LinearLayer(style_dim, out_channel, bias_init=0, std_init=0.25)

    def forward(self, input, style):
        batch, features = style.shape
        shape = (batch,) + (1,) * (input.dim() - 2) + (features,)
        gamma = self.gamma(style).view(shape)
        beta = self.beta(style).view(shape)
        # film_linear(): the reference's ops, or for the MLP's training shapes the GEMM
        # with the activation fused on the HIP kernels (linear.py, ngp network only)
        return film_linear(input, self.weight, self.bias, gamma, beta, self.train_kernels,
                           self.double_backward)


# ---------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------
class SirenGenerator(nn.Module):
    """FiLM-SIREN MLP, ``rendering.type == 'sdf'`` (sdf_model.py:101-139)."""

    net_kind = 1                  # index into _lib.NETWORKS: the fused kernels' "siren"

    def __init__(self, D=8, W=256, style_dim=256, input_ch=3, input_ch_views=3, output_ch=4,
                 output_features=True):
        super().__init__()
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = input_ch, input_ch_views
        self.style_dim = style_dim
        self.output_features = output_features
        layers = [FiLMSiren(3, W, style_dim=style_dim, is_first=True)]
        layers += [FiLMSiren(W, W, style_dim=style_dim) for _ in range(D - 1)]
        self.pts_linears = nn.ModuleList(layers)
        self.views_linears = FiLMSiren(input_ch_views + W, W, style_dim=style_dim)
        self.rgb_linear = LinearLayer(W, 3, freq_init=True)
        self.sigma_linear = LinearLayer(W, 1, freq_init=True)
        # training GEMMs on the split-fp16 kernels, double-differentiable (the eikonal
        # loss reaches these weights through autograd.grad(create_graph=True), linear.py)
        for m in [*self.pts_linears, self.views_linears, self.rgb_linear, self.sigma_linear]:
            m.train_kernels = True
            m.double_backward = True

    def forward(self, x, styles):
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        h = pts.contiguous()
        for layer in self.pts_linears:
            h = layer(h, styles)
        sdf = self.sigma_linear(h)
        feat = self.views_linears(torch.cat([h, views], -1), styles)
        rgb = self.rgb_linear(feat)
        out = torch.cat([rgb, sdf], -1)
        return torch.cat([out, feat], -1) if self.output_features else out


def get_encoder(encoding, input_dim=3, multires=6, degree=4, num_levels=16, level_dim=2,
                base_resolution=16, log2_hashmap_size=19, desired_resolution=2048,
                align_corners=False, **kwargs):
    """(encoder module, output dim) as sdf_model.py:1512-1531."""
    if encoding == "sphere_harmonics":
        enc = SHEncoder(input_dim=input_dim, degree=degree)
    elif encoding == "hashgrid":
        enc = GridEncoder(input_dim=input_dim, num_levels=num_levels, level_dim=level_dim,
                          base_resolution=base_resolution, log2_hashmap_size=log2_hashmap_size,
                          desired_resolution=desired_resolution, gridtype="hash",
                          align_corners=align_corners)
    else:
        raise NotImplementedError(
            "Unknown encoding mode, choose from [None, frequency, sphere_harmonics, hashgrid, "
            "tiledgrid]")
    return enc, enc.output_dim


class NGPSIRENGenerator(nn.Module):
    """Hash-grid + FiLM-SIREN field, ``rendering.type == 'ngp'`` (sdf_model.py:1534-1596)."""

    net_kind = 0                  # index into _lib.NETWORKS: the fused kernels' "ngp"

    def __init__(self, D=2, W=256, style_dim=256, output_features=True):
        super().__init__()
        self.D, self.W = D, W
        self.bound = 2
        self.style_dim = style_dim
        self.input_ch = 3
        self.input_ch_views = 3
        self.output_features = output_features
        self.encoder, self.in_dim = get_encoder("hashgrid", desired_resolution=2048 * self.bound)
        self.encoder_dir, self.in_dim_dir = get_encoder("sphere_harmonics")
        # the reference aliases input_linear and rgb_linear here and re-creates
        # rgb_linear below (sdf_model.py:1549, 1561); keep that RNG order and
        # the module registration order (optimizer parameter order)
        self.input_linear = LinearLayer(self.in_dim, self.W, freq_init=True)
        self.rgb_linear = self.input_linear
        layers = [FiLMSiren(self.W, self.W, style_dim=style_dim, is_first=True)]
        layers += [FiLMSiren(self.W, self.W, style_dim=style_dim) for _ in range(self.D)]
        self.pts_linears = nn.ModuleList(layers)
        self.views_linears = FiLMSiren(self.in_dim_dir + self.W, self.W, style_dim=style_dim)
        self.rgb_linear = LinearLayer(self.W, 3, freq_init=True)
        self.sigma_linear = LinearLayer(W, 1, freq_init=True)
        # training GEMMs on the split-fp16 kernels (first-order backward suffices here:
        # the eikonal term leaves autograd in the grid encoder's backward, linear.py)
        for m in [self.input_linear, *self.pts_linears, self.views_linears, self.rgb_linear,
                  self.sigma_linear]:
            m.train_kernels = True

    def forward(self, x, styles):
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        h = self.encoder(pts, bound=self.bound)
        v = self.encoder_dir(views)
        h = self.input_linear(h.contiguous())
        for layer in self.pts_linears:
            h = layer(h, styles)
        sdf = self.sigma_linear(h)
        feat = self.views_linears(torch.cat([h, v], -1), styles)
        rgb = self.rgb_linear(feat)
        out = torch.cat([rgb, sdf], -1)
        return torch.cat([out, feat], -1) if self.output_features else out

    def query_sdf(self, input_pts, styles):
        # the reference returns the hash embedding here (sdf_model.py:1594-1596)
        return self.encoder(input_pts, bound=self.bound)


class FCGenerator(nn.Module):
    """Positional-encoding ReLU MLP, ``rendering.fc == 1`` (sdf_model.py:1599-1670).
    Inference on the GPU (no gradients) runs the fused HIP renderer
    (``sdfr_render_fc_forward``); with gradients its 60-wide x_in, seven 256 -> 256,
    280-wide views layers and the sigma / rgb heads run on the split-fp16 training
    GEMMs (``linear.linear``; twice-differentiable: the eikonal term differentiates
    through them with create_graph); the per-face style_in (2 rows) stays on F.linear.
    CPU tensors take F.linear throughout."""

    net_kind = 2                  # index into _lib.NETWORKS: the fused kernels' "fc"

    def __init__(self, D=8, W=256, style_dim=256, input_ch=3, input_ch_views=3, output_ch=4,
                 output_features=True):
        super().__init__()
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = input_ch, input_ch_views
        self.style_dim = style_dim
        self.output_features = output_features
        self.n_freq_posenc = 10
        self.n_freq_posenc_views = 4
        dim_embed = 3 * self.n_freq_posenc * 2
        dim_embed_view = 3 * self.n_freq_posenc_views * 2
        self.x_in = nn.Linear(dim_embed, W)
        self.style_in = nn.Linear(style_dim, W)
        self.pts_linears = nn.ModuleList([nn.Linear(W, W) for _ in range(D - 1)])
        self.views_linears = nn.Linear(dim_embed_view + W, W)
        self.rgb_linear = nn.Linear(W, 3)
        self.sigma_linear = nn.Linear(W, 1)

    def transform_points(self, p, views=False):
        p = p / 2
        L = self.n_freq_posenc_views if views else self.n_freq_posenc
        parts = []
        for i in range(L):
            parts.append(torch.cat([torch.sin((2 ** i) * np.pi * p),
                                    torch.cos((2 ** i) * np.pi * p)], dim=-1))
        return torch.cat(parts, dim=-1)

    def forward(self, x, styles):
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        pts = self.transform_points(pts)
        views = self.transform_points(views, True)
        h = linear(pts, self.x_in.weight, self.x_in.bias, twice=True)
        s = self.style_in(styles)
        s = s.view((s.shape[0],) + (1,) * (h.dim() - 2) + (s.shape[-1],))
        h = F.relu(h + s)
        for layer in self.pts_linears:
            h = F.relu(linear(h, layer.weight, layer.bias, twice=True))
        sdf = linear(h, self.sigma_linear.weight, self.sigma_linear.bias, twice=True)
        feat = linear(torch.cat([h, views], -1), self.views_linears.weight,
                      self.views_linears.bias, twice=True)
        rgb = linear(feat, self.rgb_linear.weight, self.rgb_linear.bias, twice=True)
        out = torch.cat([rgb, sdf], -1)
        return torch.cat([out, feat], -1) if self.output_features else out


# ---------------------------------------------------------------------------
# renderer
# ---------------------------------------------------------------------------
def _opt(opt, key, default=None):
    try:
        return opt[key]
    except (KeyError, TypeError):
        return getattr(opt, key, default)


def _unit(x, dim):
    """``x / max(|x|, 1e-20)`` along ``dim`` (a zero vector stays zero)."""
    return x / x.norm(dim=dim, keepdim=True).clamp_min(1e-20)


# What VolumeFeatureRenderer.render_geometry returns: NCHW maps and the per-sample SDF and
# eikonal term in forward's layout; fields that were not asked for are None.
Geometry = namedtuple("Geometry", ("normal", "depth", "xyz", "mask", "sdf", "eikonal"))

# What VolumeFeatureRenderer.render_surface returns: NCHW maps of the SDF's first zero
# crossing along each ray (``sample`` int32, the others fp32) and the coarse per-sample SDF
# in forward's layout; fields that were not asked for are None.
Surface = namedtuple("Surface", ("hit", "sample", "depth", "xyz", "normal", "rgb", "residual",
                                 "sdf"))


class VolumeFeatureRenderer(FusedCalls, nn.Module):
    """Drop-in for sdf_model.py:143-423 (same options, buffers, outputs).  The fused HIP
    path (``fused_forward`` and the library calls behind ``query``, ``query_gradient``,
    ``render_geometry`` and ``render_surface``) is render_calls.FusedCalls."""

    def __init__(self, opt, style_dim=256, out_im_res=64, mode="train"):
        super().__init__()
        self.test = mode != "train"
        self.perturb = _opt(opt, "perturb")
        self.offset_sampling = not _opt(opt, "no_offset_sampling")
        self.N_samples = _opt(opt, "N_samples")
        self.raw_noise_std = _opt(opt, "raw_noise_std")
        self.return_xyz = _opt(opt, "return_xyz")
        self.return_sdf = _opt(opt, "return_sdf")
        self.static_viewdirs = _opt(opt, "static_viewdirs")
        self.z_normalize = not _opt(opt, "no_z_normalize")
        self.out_im_res = out_im_res
        self.force_background = _opt(opt, "force_background")
        self.with_sdf = not _opt(opt, "no_sdf")
        keys = opt.keys() if hasattr(opt, "keys") else vars(opt).keys()
        self.output_features = "no_features_output" not in keys
        if self.with_sdf:
            self.sigmoid_beta = nn.Parameter(0.1 * torch.ones(1))

        lin = torch.linspace(0.5, self.out_im_res - 0.5, self.out_im_res)
        i, j = torch.meshgrid(lin, lin, indexing="ij")
        self.register_buffer("i", i.t().unsqueeze(0), persistent=False)
        self.register_buffer("j", j.t().unsqueeze(0), persistent=False)
        if self.offset_sampling:
            t_vals = torch.linspace(0., 1. - 1 / self.N_samples, steps=self.N_samples)
        else:
            t_vals = torch.linspace(0., 1., steps=self.N_samples)
        self.register_buffer("t_vals", t_vals.view(1, 1, 1, -1), persistent=False)
        self.register_buffer("inf", torch.Tensor([1e10]), persistent=False)
        self.register_buffer("zero_idx", torch.LongTensor([0]), persistent=False)
        if self.test:
            self.perturb = False
            self.raw_noise_std = 0.

        self.channel_dim = -1
        self.samples_dim = 3
        self.input_ch = 3
        self.input_ch_views = 3
        rtype = _opt(opt, "type")
        self.feature_out_size = _opt(opt, "width") if rtype != "ngp" else style_dim
        if rtype == "ngp":
            self.network = NGPSIRENGenerator(D=2, W=style_dim, style_dim=style_dim,
                                             output_features=self.output_features)
        elif _opt(opt, "fc"):
            self.network = FCGenerator(D=_opt(opt, "depth"), W=_opt(opt, "width"),
                                       style_dim=style_dim, input_ch=self.input_ch, output_ch=4,
                                       input_ch_views=self.input_ch_views,
                                       output_features=self.output_features)
        else:
            self.network = SirenGenerator(D=_opt(opt, "depth"), W=_opt(opt, "width"),
                                          style_dim=style_dim, input_ch=self.input_ch,
                                          output_ch=4, input_ch_views=self.input_ch_views,
                                          output_features=self.output_features)
        # MI355X additions (not in the reference): where the per-ray sampling
        # offsets are drawn ('cpu' = the reference's CPU RNG stream, 'device' =
        # torch.cuda RNG, no host round trip) and a switch for the fused path.
        self.rng_device = "cpu"
        self.use_fused = True
        # field-stage GEMM arithmetic of the fused path: "f16x3" (three fp16 MFMA
        # terms on row-scaled hi/lo splits, fp32-level accuracy) or "fp32"
        # (v_mfma_f32_16x16x4_f32); include/sdfr.h, DESIGN.md section 5
        self.field_precision = "f16x3"
        # optional 4 torch.cuda.Event(enable_timing=True) recorded around the
        # fused stages (prep | hash grid | field | end), see include/sdfr.h
        self.stage_events = None
        self.field_event = None        # hipEvent recorded right before the field kernel
        # upper bound on the per-ray sample segments of the fused field stage at small
        # batches (0 = the library default 4; 1 = whole rays), include/sdfr.h
        self.max_field_segments = 0

    # ---------------------------------------------------------------- reference structure
    def get_rays(self, focal, c2w):
        dirs = torch.stack([(self.i - self.out_im_res * .5) / focal,
                            -(self.j - self.out_im_res * .5) / focal,
                            -torch.ones_like(self.i).expand(focal.shape[0], self.out_im_res,
                                                            self.out_im_res)], -1)
        # torch.sum over the 3-wide last dim (sdf_model.py:213) as its explicit
        # left-to-right form: what torch-CPU computes, and the same on every device
        # (a GPU reduction may round differently, which the 4096-resolution hash
        # level turns into different cells; tests pin it against the golden rays)
        prod = dirs[..., None, :] * c2w[:, None, None, :3, :3]
        rays_d = prod[..., 0] + prod[..., 1] + prod[..., 2]
        rays_o = c2w[:, None, None, :3, -1].expand(rays_d.shape)
        viewdirs = dirs if self.static_viewdirs else rays_d
        return rays_o, rays_d, viewdirs

    def get_eikonal_term(self, pts, sdf):
        # only d sdf / d pts is returned: the grid encoder and the training GEMMs skip
        # the gradients this pass does not use (linear._wanted)
        return autograd.grad(outputs=sdf, inputs=pts, grad_outputs=torch.ones_like(sdf),
                             create_graph=True)[0]

    def sdf_activation(self, input):
        return torch.sigmoid(input / self.sigmoid_beta) / self.sigmoid_beta

    def compositing_weights(self, sdf, z_vals, rays_d, noise=0.):
        """The weights [B,H,W,N,1] of the front-to-back composite (sdf_model.py:236-301)
        from the network's per-sample fourth output [B,H,W,N,1]: the SDF, or without one
        the raw density that ``noise`` is added to.  The one place that turns alpha into
        weights; autograd follows the caller's grad mode."""
        dists = z_vals[..., 1:] - z_vals[..., :-1]
        rays_d_norm = torch.norm(rays_d.unsqueeze(self.samples_dim), dim=self.channel_dim)
        dists = torch.cat([dists, self.inf.expand(rays_d_norm.shape)], self.channel_dim)
        dists = dists * rays_d_norm
        density = self.sdf_activation(-sdf) if self.with_sdf else F.softplus(sdf + noise)
        sigma = 1 - torch.exp(-density * dists.unsqueeze(self.channel_dim))
        first = torch.ones_like(torch.index_select(sigma, self.samples_dim, self.zero_idx))
        visibility = torch.cumprod(torch.cat([first, 1. - sigma + 1e-10], self.samples_dim),
                                   self.samples_dim)[..., :-1, :]
        weights = sigma * visibility
        if self.force_background:
            weights[..., -1, :] = 1 - weights[..., :-1, :].sum(self.samples_dim)
        return weights

    def volume_integration(self, raw, z_vals, rays_d, pts, return_eikonal=False):
        if self.output_features:
            rgb, sdf, features = torch.split(raw, [3, 1, self.feature_out_size],
                                             dim=self.channel_dim)
        else:
            rgb, sdf = torch.split(raw, [3, 1], dim=self.channel_dim)
        noise = 0.
        if self.raw_noise_std > 0.:
            noise = torch.randn_like(sdf) * self.raw_noise_std
        eikonal_term = None
        if self.with_sdf and return_eikonal:
            eikonal_term = self.get_eikonal_term(pts, sdf)
        weights = self.compositing_weights(sdf, z_vals, rays_d, noise)
        sdf_out = sdf if self.return_sdf else None
        rgb_map = -1 + 2 * torch.sum(weights * torch.sigmoid(rgb), self.samples_dim)
        feature_map = (torch.sum(weights * features, self.samples_dim)
                       if self.output_features else None)
        if self.return_xyz:
            xyz = torch.sum(weights * pts, self.samples_dim)
            mask = weights[..., -1, :]
        else:
            xyz = mask = None
        return rgb_map, feature_map, sdf_out, mask, xyz, eikonal_term

    def run_network(self, inputs, viewdirs, styles=None):
        input_dirs = viewdirs.unsqueeze(self.samples_dim).expand(inputs.shape)
        return self.network(torch.cat([inputs, input_dirs], self.channel_dim), styles=styles)

    def _draw_t_rand(self, shape, device):
        if self.rng_device == "cpu":
            return torch.rand(shape).to(device)
        return torch.rand(shape, device=device)

    def render_rays(self, ray_batch, styles=None, return_eikonal=False, t_rand=None):
        split = [3, 3, 2]
        if ray_batch.shape[-1] > 8:
            rays_o, rays_d, bounds, viewdirs = torch.split(ray_batch, split + [3], dim=-1)
        else:
            rays_o, rays_d, bounds = torch.split(ray_batch, split, dim=-1)
            viewdirs = None
        near, far = torch.split(bounds, [1, 1], dim=-1)
        z_vals, pts, normalized_pts = self.sample_points(
            rays_o, rays_d, near, far, t_rand, self._stratify(), pts_grad=return_eikonal)
        raw = self.run_network(normalized_pts, viewdirs, styles=styles)
        return self.volume_integration(raw, z_vals, rays_d, pts, return_eikonal=return_eikonal)

    def camera_rays(self, focal, c2w, near, far):
        """``rays_o, rays_d, viewdirs`` (unit length) [B,H,W,3] and ``near, far`` [B,H,W,1]."""
        rays_o, rays_d, viewdirs = self.get_rays(focal, c2w)
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
        near = near.unsqueeze(-1) * torch.ones_like(rays_d[..., :1])
        far = far.unsqueeze(-1) * torch.ones_like(rays_d[..., :1])
        return rays_o, rays_d, viewdirs, near, far

    def _stratify(self):
        """The renderer's own mode of ``sample_points``."""
        if self.perturb > 0.:
            return "offset" if self.offset_sampling else "mid"
        return None

    def sample_points(self, rays_o, rays_d, near, far, t_rand, stratify, pts_grad=False):
        """``z_vals`` [B,H,W,N], the samples ``pts`` [B,H,W,N,3] and what the network sees
        of them: the one place that knows how samples are placed along a ray.
        ``stratify``: None (the ``t_vals`` depths), "offset" (one shift per ray, up to the
        next depth) or "mid" (one draw per sample between the mid-points); ``t_rand`` is
        drawn in that shape when it is None.  ``pts_grad``: ``pts`` requires grad, for the
        eikonal term."""
        z_vals = near * (1. - self.t_vals) + far * self.t_vals
        if stratify is not None:
            if stratify == "offset":
                upper = torch.cat([z_vals[..., 1:], far], -1)
                lower = z_vals.detach()
                drawn, shape = z_vals.shape[:-1], z_vals.shape[:-1] + (1,)
            else:
                mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
                upper = torch.cat([mids, z_vals[..., -1:]], -1)
                lower = torch.cat([z_vals[..., :1], mids], -1)
                drawn = shape = z_vals.shape
            if t_rand is None:
                t_rand = self._draw_t_rand(drawn, z_vals.device)
            z_vals = lower + (upper - lower) * t_rand.to(z_vals.device).reshape(shape)
        pts = rays_o.unsqueeze(3) + rays_d.unsqueeze(3) * z_vals.unsqueeze(-1)
        if pts_grad:
            pts.requires_grad = True
        normalized_pts = pts * 2 / ((far - near).unsqueeze(3)) if self.z_normalize else pts
        return z_vals, pts, normalized_pts

    def render(self, focal, c2w, near, far, styles, c2w_staticcam=None, return_eikonal=False,
               t_rand=None):
        rays_o, rays_d, viewdirs, near, far = self.camera_rays(focal, c2w, near, far)
        rays = torch.cat([rays_o, rays_d, near, far], -1)
        rays = torch.cat([rays, viewdirs], -1).float()
        return self.render_rays(rays, styles=styles, return_eikonal=return_eikonal,
                                t_rand=t_rand)

    def mlp_init_pass(self, cam_poses, focal, near, far, styles=None, t_rand=None):
        rays_o, rays_d, viewdirs, near, far = self.camera_rays(focal, cam_poses, near, far)
        # always one draw per sample, whatever perturb and offset_sampling say
        _, pts, normalized_pts = self.sample_points(rays_o, rays_d, near, far, t_rand, "mid")
        raw = self.run_network(normalized_pts, viewdirs, styles=styles)
        _, sdf = torch.split(raw[..., :4], [3, 1], dim=-1)
        sdf = sdf.squeeze(-1)
        target_values = pts.detach().norm(dim=-1) - ((far - near) / 4)
        return sdf, target_values

    # ---------------------------------------------------------------- point query
    def query(self, points, styles, viewdirs=None, return_rgb=True, chunk_groups=None):
        """The field itself at arbitrary points: ``(sdf [B,M], rgb [B,M,3] | None)``.

        ``points`` [B,M,3] are NETWORK coordinates (what ``self.network`` receives: a
        world position times ``2 / (far - near)`` under z-normalisation, see
        ``mesh.world_to_network``).  ``sdf`` is sigma_linear's output, ``rgb`` is
        sigmoid(rgb_linear) in [0,1] -- the per-sample values the render composites.
        ``viewdirs`` is the view direction as the network sees it (unit length; it is
        not normalised here): ``[B,3]`` one per face, ``[B,M,3]`` one per point, or
        ``None`` with ``return_rgb=False`` (zeros are passed).

        For CUDA tensors, ``field_precision == 'f16x3'`` and no grad needed this runs
        ``sdfr_query_ngp_forward`` / ``sdfr_query_siren_forward`` / ``sdfr_query_fc_forward``:
        the render's split-fp16 field kernel (for ngp behind the render's hash-grid
        gather) on the given points, so a point the render samples gets the render's SDF
        bit for bit.  Per-face (or no) directions run in groups of N = 32 points (M
        padded, the padding trimmed); per-point directions run as M groups of N = 1,
        which idles the kernel's other sample lanes (ngp and FC take 2 points of a group
        per pass: half rate; SIREN takes 4: quarter rate).  Calls are chunked over groups
        (``chunk_groups``, default ``QUERY_CHUNK_POINTS`` / N) to bound the workspace;
        chunking does not change a bit of the result.  The SIREN kernel splits each
        coordinate into fp16 hi + lo parts unscaled, as its render does: coordinates
        must stay below fp16's 65504, and the accuracy tests cover |coordinate| <= 64,
        the supported range (the render's samples stay below 1.3).  Otherwise (CPU
        tensors, the fp32 field, a call under grad, a SIREN or FC network of another
        depth or width) it runs ``self.network(cat([points, dirs]), styles)``, the autograd
        path, and slices it.
        """
        if points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError(f"query: points must be [B,M,3], got {tuple(points.shape)}")
        B, M = points.shape[:2]
        if viewdirs is None:
            if return_rgb:
                raise ValueError("query: return_rgb needs viewdirs")
            viewdirs = points.new_zeros(B, 3)
        per_point = viewdirs.dim() == 3
        if tuple(viewdirs.shape) != ((B, M, 3) if per_point else (B, 3)):
            raise ValueError(f"query: viewdirs must be [B,3] or [B,M,3] for points "
                             f"{tuple(points.shape)}, got {tuple(viewdirs.shape)}")
        if not self._query_fused_ok(points, styles):
            dirs = viewdirs if per_point else viewdirs.unsqueeze(1).expand(B, M, 3)
            raw = self.network(torch.cat([points, dirs.to(points)], -1), styles=styles)
            return raw[..., 3], (torch.sigmoid(raw[..., :3]) if return_rgb else None)
        # groups of N points sharing a direction: [B,R,N,3] points, [B,R,3] directions
        N = 1 if per_point else 32
        R = (M + N - 1) // N
        pts = points.detach().float()
        if R * N != M:
            pts = torch.cat([pts, pts.new_zeros(B, R * N - M, 3)], 1)
        dirs = viewdirs.detach().to(device=points.device, dtype=torch.float32)
        dirs = dirs if per_point else dirs.unsqueeze(1).expand(B, R, 3)
        sdf, rgb = self._fused_query(pts.reshape(B, R, N, 3), dirs, styles, return_rgb,
                                     chunk_groups)
        sdf = sdf.reshape(B, R * N)[:, :M]
        return sdf, (rgb.reshape(B, R * N, 3)[:, :M] if return_rgb else None)

    # ---------------------------------------------------------------- SDF gradient
    def query_gradient(self, points, styles, normalize=False, chunk_points=None,
                       encode_only=False):
        """The SDF and its gradient at arbitrary points: ``(sdf [B,M], grad [B,M,3])``.

        ``points`` [B,M,3] are NETWORK coordinates as for ``query``; ``grad`` is
        d sdf / d point in the same coordinates (times ``2 / (far - near)`` for a world
        gradient, see ``mesh.eikonal_residual``).  ``normalize=True`` returns
        ``grad / max(|grad|, 1e-20)`` (unit rows; a zero gradient stays zero).

        Under the rule of ``query``'s fused path this runs ``sdfr_query_ngp_grad`` (ngp:
        a hash-grid gather that also stores the input derivatives, and a forward-mode
        split-fp16 field kernel over the SDF trunk -- the exact gradient of the piecewise
        trilinear field, ``sdf`` bit-identical to ``query``'s) or ``sdfr_query_siren_grad``
        (SIREN: the same forward-mode kernel over the eight FiLM layers with the point and
        the three unit vectors as layer 0's columns, on a packing of the trunk of its own;
        ``sdf`` equals ``query``'s up to fp32 rounding, the accumulation order differs) or
        ``sdfr_query_fc_grad`` (FC: the same kernel over x_in and the seven ReLU layers on
        the render's own packing, layer 0's columns being the positional encodings and
        their derivatives; a tangent passes a ReLU where the value's pre-activation is
        > 0, as ``torch.relu``'s backward has it; ``sdf`` bit-identical to ``query``'s).
        No autograd graph is built.  Calls
        are chunked over points (``chunk_points`` per face, rounded down to the kernel's
        workgroup pass of 32 points; default ``GRADIENT_CHUNK_POINTS`` / B) to bound the
        workspace; chunking does not change a bit of the result.  Otherwise (CPU
        tensors, the fp32 field, grad mode with a tensor or parameter that requires grad)
        it is ``torch.autograd.grad(sdf.sum(), points)``
        through ``self.network`` with zero view directions, on a detached copy of the
        points with grad enabled locally -- so it also works under ``no_grad``, and the
        caller's ``points`` are left alone.  Either way the result carries no autograd
        graph (an inference query).

        ``encode_only=True`` (ngp fused path only) returns the gather's output instead:
        ``(features [B,M,32], dy_du [B,M,3,32])``, feature index 2 level + c.  A SIREN
        or FC network has no hash-grid gather: ``ValueError``.
        """
        if points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError(f"query_gradient: points must be [B,M,3], got {tuple(points.shape)}")
        if encode_only and self._net_kind() != 0:
            raise ValueError("query_gradient: encode_only returns the ngp hash-grid gather's "
                             "output; this network has no hash grid")
        fused = self._query_fused_ok(points, styles)
        if encode_only and not fused:
            raise ValueError("query_gradient: encode_only needs the fused path")
        if fused:
            out = self._fused_gradient(points, styles, chunk_points, encode_only)
            if encode_only:
                return out
            sdf, grad = out
        else:
            with torch.enable_grad():
                pts = points.detach().clone().requires_grad_(True)
                raw = self.network(torch.cat([pts, torch.zeros_like(pts)], -1),
                                   styles=styles.detach())
                sdf = raw[..., 3]
                grad, = torch.autograd.grad(sdf.sum(), pts)
            sdf = sdf.detach()
        return sdf, (_unit(grad, -1) if normalize else grad)

    # ---------------------------------------------------------------- geometry render
    GEOMETRY_FIELDS = ("normal", "depth", "xyz", "mask", "sdf", "eikonal")

    def render_geometry(self, cam_poses, focal, near, far, styles, t_rand=None,
                        want=("normal", "depth", "xyz", "mask"), normalize=False,
                        chunk_points=None):
        """The geometry of a render: ``Geometry(normal, depth, xyz, mask, sdf, eikonal)``
        for the cameras of ``forward``; fields not named in ``want`` are ``None``.

        ``sdf`` [B,H,W,N,1] and ``eikonal`` [B,H,W,N,3] are the per-sample SDF and its
        gradient with respect to the world point, as ``forward(return_eikonal=True)``
        returns them (sdf_model.py:224-229).  ``normal`` [B,3,H,W] (sum of w eikonal, not
        normalised unless ``normalize``: then divided by ``max(|normal|, 1e-20)``),
        ``depth`` [B,1,H,W] (sum of w z), ``xyz`` [B,3,H,W] and ``mask`` [B,1,H,W] are
        composited with exactly the render's weights.  The sampling flags (``perturb``,
        ``offset_sampling``, ``z_normalize``, ``force_background``, ``N_samples``,
        ``out_im_res``) are the renderer's; ``t_rand`` is drawn as in ``forward`` when
        ``perturb > 0`` and none is given.

        Under the rule of ``query_gradient``'s fused path this runs
        ``sdfr_render_ngp_geometry`` (the sample points, the gradient call's gather and
        forward-mode field kernel, a compositing kernel; ``sdf`` is the fused render's
        ``return_sdf`` output bit for bit), in calls of at most ``chunk_points`` points
        (default ``GRADIENT_CHUNK_POINTS``) over faces and bands of whole image rows; a
        single row above the chunk is one call.  Chunking does not change a bit of any
        output.  Otherwise (SIREN and FC -- the fused geometry render is ngp's --, CPU
        tensors, the fp32 field, grad mode with
        something that requires grad) the same definitions are computed op by op, the
        gradient by autograd with grad enabled locally on detached inputs.  Either way the
        result carries no autograd graph.
        """
        if not self.with_sdf:
            raise ValueError("render_geometry: the renderer has no SDF (no_sdf)")
        want = tuple(want)
        unknown = [k for k in want if k not in self.GEOMETRY_FIELDS]
        if unknown or not want:
            raise ValueError(f"render_geometry: want must name some of "
                             f"{self.GEOMETRY_FIELDS}, got {want}")
        if self._net_kind() == 0 and self._query_fused_ok(cam_poses, styles):
            out = self._fused_geometry(cam_poses, focal, near, far, styles, t_rand, want,
                                       chunk_points)
        else:
            out = self._module_geometry(cam_poses, focal, near, far, styles, t_rand, want)
        if normalize and out.get("normal") is not None:
            out["normal"] = _unit(out["normal"], 1)
        return Geometry(**{k: out.get(k) for k in self.GEOMETRY_FIELDS})

    def _module_geometry(self, cam_poses, focal, near, far, styles, t_rand, want):
        """``render_geometry`` op by op: the rays, samples and weights of ``render``, the
        gradient by autograd on detached inputs."""
        cam_poses, focal, near, far = (t.detach() for t in (cam_poses, focal, near, far))
        styles = styles.detach() if styles is not None else None
        with torch.no_grad():
            rays_o, rays_d, viewdirs, near, far = (
                t.float() for t in self.camera_rays(focal, cam_poses, near, far))
        with torch.enable_grad():
            z_vals, pts, normalized_pts = self.sample_points(
                rays_o, rays_d, near, far, t_rand, self._stratify(), pts_grad=True)
            raw = self.run_network(normalized_pts, viewdirs, styles=styles)
            sdf = raw[..., 3:4]
            eikonal, = autograd.grad(outputs=sdf, inputs=pts, grad_outputs=torch.ones_like(sdf))
        sdf, pts = sdf.detach(), pts.detach()
        out = {}
        if "sdf" in want:
            out["sdf"] = sdf
        if "eikonal" in want:
            out["eikonal"] = eikonal
        if any(k in want for k in ("normal", "depth", "xyz", "mask")):
            with torch.no_grad():
                weights = self.compositing_weights(sdf, z_vals, rays_d)
                maps = {"normal": lambda: torch.sum(weights * eikonal, self.samples_dim),
                        "depth": lambda: torch.sum(weights * z_vals.unsqueeze(-1),
                                                   self.samples_dim),
                        "xyz": lambda: torch.sum(weights * pts, self.samples_dim),
                        "mask": lambda: weights[..., -1, :]}
                for k, fn in maps.items():
                    if k in want:
                        out[k] = fn().permute(0, 3, 1, 2).contiguous()
        return out

    # ---------------------------------------------------------------- surface render
    SURFACE_FIELDS = Surface._fields

    def render_surface(self, cam_poses, focal, near, far, styles, t_rand=None, refine_steps=8,
                       want=("hit", "depth", "xyz", "normal", "rgb"), chunk_points=None):
        """The surface itself as an image: ``Surface(hit, sample, depth, xyz, normal, rgb,
        residual, sdf)`` for the cameras of ``forward``; fields not named in ``want`` are
        ``None``.  Per ray (the definition is pinned in include/sdfr.h):

        1. *Bracket*: ``s*`` is the first sample with ``sdf_s > 0`` and ``sdf_{s+1} <= 0``
           (outside -> inside) among the render's own samples and SDF.  No such sample is a
           miss.  A ray that starts inside the surface is not special-cased: its samples up
           to the first positive one are skipped, so it reports where it enters again.
        2. *Refine*: ``refine_steps`` (0..32) bisection steps on ``[z_s*, z_s*+1]``, the SDF
           of each midpoint being exactly what ``query`` returns there.  The count is fixed
           (no convergence test, no host synchronisation).
        3. *Interpolate*: ``z*`` linearly between the final bracket's ends, clamped to it.
        4. *Finish*: ``residual`` is ``query_gradient``'s SDF at the hit point, ``normal``
           its gradient with respect to the world point divided by ``max(|.|, 1e-20)``,
           ``rgb`` is ``query``'s colour there (in [0,1]) with the view direction the
           render gives the network for the ray.

        ``hit`` [B,1,H,W] is 1.0 / 0.0, ``sample`` [B,1,H,W] int32 is ``s*`` or -1, ``depth``
        [B,1,H,W] is ``z*``, ``xyz`` [B,3,H,W] the world point ``o + d z*``, ``normal`` and
        ``rgb`` [B,3,H,W], ``sdf`` [B,H,W,N,1] the coarse SDF in forward's layout.  On a
        miss every float map is 0.  The sampling flags are the renderer's; ``t_rand`` is
        drawn as in ``forward`` when ``perturb > 0`` and none is given.

        For an ngp or SIREN network under the rule of ``query``'s fused path this runs
        ``sdfr_render_ngp_surface`` / ``sdfr_render_siren_surface`` in calls of at most
        ``chunk_points`` samples (default ``SURFACE_CHUNK_POINTS``) over faces and bands of
        whole image rows; rays are independent, so chunking does not change a bit.
        Otherwise (FC, CPU tensors, the fp32 field, grad mode with something that requires
        grad) ``_module_surface`` computes the same definition op by op on
        ``self.network``.  Either way the result carries no autograd graph.
        """
        if not self.with_sdf:
            raise ValueError("render_surface: the renderer has no SDF (no_sdf)")
        want = tuple(want)
        unknown = [k for k in want if k not in self.SURFACE_FIELDS]
        if unknown or not want:
            raise ValueError(f"render_surface: want must name some of "
                             f"{self.SURFACE_FIELDS}, got {want}")
        refine_steps = int(refine_steps)
        if not 0 <= refine_steps <= 32:
            raise ValueError(f"render_surface: refine_steps must be 0..32, got {refine_steps}")
        # (the fused surface render is ngp's and SIREN's; FC has the fused point calls only)
        fused = self._net_kind() in (0, 1) and self._query_fused_ok(cam_poses, styles)
        path = self._fused_surface if fused else self._module_surface
        out = path(cam_poses, focal, near, far, styles, t_rand, refine_steps, want, chunk_points)
        return Surface(**{k: out.get(k) for k in self.SURFACE_FIELDS})

    def _module_surface(self, cam_poses, focal, near, far, styles, t_rand, refine_steps, want,
                        chunk_points=None):
        """``render_surface`` op by op on ``self.network``: the definition in code.  Every
        line is one rounded fp32 operation of the definition's chain; the gradient is
        autograd's, with grad enabled locally on detached inputs."""
        cam_poses, focal, near, far = (t.detach() for t in (cam_poses, focal, near, far))
        styles = styles.detach() if styles is not None else None
        with torch.no_grad():
            rays_o, rays_d, viewdirs, near, far = (
                t.float() for t in self.camera_rays(focal, cam_poses, near, far))
            z_vals, _, normalized_pts = self.sample_points(rays_o, rays_d, near, far, t_rand,
                                                           self._stratify())
            sdf = self.run_network(normalized_pts, viewdirs, styles=styles)[..., 3]
            N = sdf.shape[-1]
            span = far - near                                      # [B,H,W,1]

            def network_point(z):
                p = rays_o + rays_d * z.unsqueeze(-1)
                return p, (p * 2 / span if self.z_normalize else p)

            def field(p_net):
                return self.network(torch.cat([p_net, viewdirs], -1), styles=styles)

            # 1. bracket: the first s with sdf_s > 0 >= sdf_{s+1}
            if N > 1:
                cross = (sdf[..., :-1] > 0) & (sdf[..., 1:] <= 0)
                steps = torch.arange(N - 1, device=sdf.device).expand(cross.shape)
                first = torch.where(cross, steps, torch.full_like(steps, N)).min(-1).values
            else:
                first = torch.full(sdf.shape[:-1], N, dtype=torch.long, device=sdf.device)
            hit = first < N
            s0 = torch.where(hit, first, torch.zeros_like(first)).unsqueeze(-1)
            s1 = (s0 + 1).clamp_max(N - 1)
            a, b = z_vals.expand(sdf.shape).gather(-1, s0)[..., 0], \
                z_vals.expand(sdf.shape).gather(-1, s1)[..., 0]
            fa, fb = sdf.gather(-1, s0)[..., 0], sdf.gather(-1, s1)[..., 0]
            # 2. refine: a fixed number of bisection steps
            for _ in range(refine_steps):
                m = 0.5 * (a + b)
                f = field(network_point(m)[1])[..., 3]
                pos = f > 0
                a, fa = torch.where(pos, m, a), torch.where(pos, f, fa)
                b, fb = torch.where(pos, b, m), torch.where(pos, fb, f)
            # 3. interpolate (a miss keeps a valid point: its bracket's near end)
            t = torch.where(hit, fa / (fa - fb), torch.zeros_like(fa))
            z = torch.minimum(torch.maximum(a + t * (b - a), a), b)
            p, p_net = network_point(z)
        mask = hit.unsqueeze(1)                                    # [B,1,H,W]

        def nchw(v):
            v = v.unsqueeze(-1) if v.dim() == 3 else v
            v = v.permute(0, 3, 1, 2)
            return torch.where(mask, v, torch.zeros_like(v)).contiguous()

        out = {}
        if "sdf" in want:
            out["sdf"] = sdf.unsqueeze(-1)
        if "hit" in want:
            out["hit"] = mask.float()
        if "sample" in want:
            out["sample"] = torch.where(hit, first, -torch.ones_like(first)).int().unsqueeze(1)
        if "depth" in want:
            out["depth"] = nchw(z)
        if "xyz" in want:
            out["xyz"] = nchw(p)
        # 4. finish
        if "normal" in want or "residual" in want:
            with torch.enable_grad():
                pts = p_net.detach().clone().requires_grad_(True)
                res = self.network(torch.cat([pts, torch.zeros_like(pts)], -1),
                                   styles=styles)[..., 3]
                g, = torch.autograd.grad(res.sum(), pts)
            e = g * 2 / span if self.z_normalize else g
            if "residual" in want:
                out["residual"] = nchw(res.detach())
            if "normal" in want:
                out["normal"] = nchw(_unit(e, -1))
        if "rgb" in want:
            with torch.no_grad():
                out["rgb"] = nchw(torch.sigmoid(field(p_net)[..., :3]))
        return out

    # ---------------------------------------------------------------- API
    def forward(self, cam_poses, focal, near, far, styles=None, return_eikonal=False,
                t_rand=None, styles_event=None, feat_mod=None):
        """``feat_mod``: see fused_forward (the module path returns NCHW features)."""
        if self._fused_ok(cam_poses, styles, return_eikonal):
            return self.fused_forward(cam_poses, focal, near, far, styles, t_rand=t_rand,
                                      styles_event=styles_event, feat_mod=feat_mod)
        if styles_event is not None:
            torch.cuda.current_stream(cam_poses.device).wait_event(styles_event)
        rgb, features, sdf, mask, xyz, eikonal_term = self.render(
            focal, c2w=cam_poses, near=near, far=far, styles=styles,
            return_eikonal=return_eikonal, t_rand=t_rand)
        rgb = rgb.permute(0, 3, 1, 2).contiguous()
        if self.output_features:
            features = features.permute(0, 3, 1, 2).contiguous()
        if xyz is not None:
            xyz = xyz.permute(0, 3, 1, 2).contiguous()
            mask = mask.permute(0, 3, 1, 2).contiguous()
        return rgb, features, sdf, mask, xyz, eikonal_term

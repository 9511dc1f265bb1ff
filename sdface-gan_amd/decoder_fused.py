"""The decoder's fused inference path: what ``Decoder`` (generator.py) needs to run its
layers on the HIP kernels of decoder_ops.py.  ``FusedDecoder`` is the mixin
the decoder inherits; ``DecoderPlan`` is everything that path derives from the weights, built
once per weight version; ``Prepared`` / ``Styles`` are what ``prepare_fused`` hands to
``forward``.

The fused path runs where ``sdfr_decoder_styles`` -- its only style prep -- can take the
decoder: a latent width of 256 or 512 and at most 16 stacked modulation layers and 16
demodulated layers.  Any other decoder runs the module path (``Decoder._forward``), which is
the reference semantics; ``fused_ready`` is False for it.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

from . import _lib
from .decoder_ops import (conv3x3_f16x3, conv3x3_f16x3_act, conv_pack_weights, conv_t_act,
                          modulate_to_nhwc, modulate_to_nhwc_split, rgb_finish,
                          separable_taps, styled_epilogue)

Prepared = namedtuple("Prepared", "latent noise styles")


class Styles(namedtuple("Styles", "mods rgb_mods demods")):
    """Every layer's modulation [B, Cin] (``mods`` per conv, ``rgb_mods`` per ToRGB) and
    every split-fp16 layer's demodulation / su [B, Cout] (``demods``: layer -> tensor)."""
    __slots__ = ()

    def rows(self, sl):
        """Faces ``sl`` of every modulation and demodulation."""
        return Styles([m[sl] for m in self.mods], [m[sl] for m in self.rgb_mods],
                      {i: d[sl] for i, d in self.demods.items()})


class _Layer:
    """One StyledConv of the plan (the weight-derived members are set by ``load``)."""
    __slots__ = ("sc", "cin", "cout", "upsample", "split", "to_rgb", "packed", "su",
                 "rgb_base")

    def __init__(self, sc, split, to_rgb):
        self.sc, self.split, self.to_rgb = sc, split, to_rgb
        self.cout, self.cin = sc.conv.weight.shape[1:3]
        self.upsample = sc.conv.upsample
        self.packed = self.su = self.rgb_base = None


def _plan_tensors(dec):
    """The tensors a plan derives data from: every conv's weight with its modulation's
    weight and bias, and the blur kernels."""
    ts = []
    for m in [dec.conv1, *dec.convs, dec.to_rgb1, *dec.to_rgbs]:
        mc = m.conv                  # (a module's attribute lookup is the cost of the key)
        lin = mc.modulation
        ts += (mc.weight, lin.weight, lin.bias)
    blurs = []
    if len(dec.convs):
        blurs = [dec.convs[0].conv.blur.kernel] + [t.upsample.kernel for t in dec.to_rgbs]
    return ts, blurs


class DecoderPlan:
    """What the fused path derives from one version of a decoder's weights.  Building it
    reads shapes and the blur kernels only (any device); ``load`` adds the tensors.  A plain
    object: nothing it holds is a parameter or buffer of the decoder, and it does not refer
    back to the decoder."""

    def __init__(self, dec, key, prev=None):
        self.key = key
        seq = [dec.conv1] + list(dec.convs)
        rgbs = [dec.to_rgb1] + list(dec.to_rgbs)
        # ToRGB k follows conv 2k and reads latent 2k + 1
        self.layers = [_Layer(sc, self._splits(sc.conv, dec.conv_impl),
                              rgbs[i // 2] if i % 2 == 0 else None)
                       for i, sc in enumerate(seq)]
        self.seq = seq
        # the one 4-tap filter every blur and ToRGB upsample shares, or None; reading the
        # kernels synchronises with the device, so the taps of the plan before this one are
        # kept while the blur kernels' part of the key stands
        if prev is not None and prev.key[2] == key[2]:
            self.fir = prev.fir
        else:
            fir = separable_taps(seq[1].conv.blur.kernel) if len(seq) > 1 else [0.0] * 4
            if fir is not None and not all(
                    torch.equal(t.upsample.kernel.cpu(), seq[1].conv.blur.kernel.cpu())
                    for t in rgbs[1:]):
                fir = None
            self.fir = fir
        # stacked modulations: the convs', then the ToRGBs'
        self.lins = [sc.conv.modulation for sc in seq] + [t.conv.modulation for t in rgbs]
        self.mod_index = list(range(len(seq))) + [2 * k + 1 for k in range(len(rgbs))]
        self.mod_c = [m.weight.shape[0] for m in self.lins]
        self.cmax = max(256, max(self.mod_c))
        self.K = self.lins[0].weight.shape[1]
        self.dem_layer = [i for i, ly in enumerate(self.layers) if ly.split]
        self.dem_c = [self.layers[i].cout for i in self.dem_layer]
        self.loaded = False

    def __reduce__(self):
        # a copied or unpickled decoder builds its own plan (this one holds device pointers)
        return type(None), ()

    @staticmethod
    def _splits(mc, conv_impl):
        """Does this ModulatedConv2d run on the split-fp16 implicit GEMM?"""
        _, cout, cin, k, _ = mc.weight.shape
        return (conv_impl == "f16x3" and k == 3 and mc.demodulate and not mc.downsample
                and cout % 128 == 0 and cin % 32 == 0)

    @property
    def supported(self):
        """Can sdfr_decoder_styles and the epilogues' one filter take this decoder?  (fp32
        modulations of a 256- or 512-wide latent, the widest padded to 256 or 512, at most
        16 stacked and 16 demodulated layers.)"""
        return (self.fir is not None and self.K in (256, 512) and self.cmax in (256, 512)
                and self.lins[0].weight.dtype == torch.float32 and len(self.lins) <= 16
                and len(self.dem_layer) <= 16)

    def load(self):
        """The tensors derived from the weights, on their device, and sdfr_style_args with
        every member that does not depend on the batch: the modulation weights (x scale) and
        biases (x lr_mul) of every layer stacked, zero-padded to the widest; per ToRGB its
        scaled 1x1 weight [3, C]; and per split-fp16 layer the packed weights, their row
        scales su and, stacked for the demodulation, su^2 * sum_{ky,kx} w^2 as ``dem_w``
        [Cout, Cin] plus su^2 * 1e-8 as ``dem_eps`` -- rsqrt(s^2 @ dem_w^T + dem_eps) is demod / su
        exactly (powers of two commute with rounding).  Packing needs the GPU: from CPU
        weights only the modulation stack and the ToRGB bases are built."""
        if self.loaded:
            return self
        w0 = self.lins[0].weight
        L, J = len(self.lins), len(self.dem_layer) if w0.is_cuda else 0
        with torch.no_grad():
            self.mod_w = w0.new_zeros(L, self.cmax, self.K)
            self.mod_b = w0.new_zeros(L, self.cmax)
            for k, m in enumerate(self.lins):
                self.mod_w[k, :self.mod_c[k]] = m.weight * m.scale
                self.mod_b[k, :self.mod_c[k]] = m.bias * m.lr_mul
            for ly in self.layers:
                if ly.to_rgb is not None:
                    tc = ly.to_rgb.conv
                    ly.rgb_base = tc.scale * tc.weight[0, :, :, 0, 0]
            self.omax = max(self.dem_c, default=0)
            self.dem_w = w0.new_zeros(J, self.omax, self.cmax)
            self.dem_eps = w0.new_zeros(J, self.omax)
            for j, i in enumerate(self.dem_layer[:J]):
                ly, mc = self.layers[i], self.layers[i].sc.conv
                ly.packed, ly.su = conv_pack_weights(mc.weight[0], mc.scale)
                w = mc.scale * mc.weight[0]
                s2 = ly.su * ly.su
                self.dem_w[j, :ly.cout, :ly.cin] = (w * w).sum([2, 3]) * s2[:, None]
                self.dem_eps[j, :ly.cout] = s2 * 1e-8
        a = self.style_args = _lib.StyleArgs()
        a.K, a.L, a.cmax = self.K, L, self.cmax
        a.mod_w, a.mod_b = _lib.ptr(self.mod_w), _lib.ptr(self.mod_b)
        a.mod_index[:L], a.mod_c[:L] = self.mod_index, self.mod_c
        if J:
            a.J, a.omax = J, self.omax
            a.dem_w, a.dem_eps = _lib.ptr(self.dem_w), _lib.ptr(self.dem_eps)
            a.dem_layer[:J], a.dem_c[:J] = self.dem_layer, self.dem_c
        self.loaded = True
        return self

    @staticmethod
    def _offsets(B, widths):
        """Where each [B, width] block starts in one flat buffer, and the buffer's size."""
        offs, off = [], 0
        for c in widths:
            offs.append(off)
            off += B * c
        return offs, off

    def styles(self, latent):
        """Every modulation and demodulation of ``latent`` [B, n_latent, K] in two HIP
        launches (sdfr_decoder_styles): they come back as contiguous [B, C] slices of two
        flat buffers.  fp32, fixed summation order."""
        if not (latent.is_cuda and latent.dtype == torch.float32 and latent.dim() == 3
                and latent.shape[2] == self.K):
            raise RuntimeError("decoder: the fused path takes fp32 latents [B, n_latent, "
                               f"{self.K}] on the GPU, got {latent.dtype} "
                               f"{tuple(latent.shape)} on {latent.device}")
        B = latent.shape[0]
        lat = latent.contiguous()
        L, J = len(self.lins), len(self.dem_layer)
        a = _lib.StyleArgs.from_buffer_copy(self.style_args)
        a.B, a.n_latent, a.latent = B, lat.shape[1], _lib.ptr(lat)
        offs, total = self._offsets(B, self.mod_c)
        a.mod_off[:L] = offs
        mflat = torch.empty(total, device=lat.device)
        a.mods = _lib.ptr(mflat)
        doffs, dtotal = self._offsets(B, self.dem_c)
        dflat = torch.empty(dtotal, device=lat.device) if J else None
        a.dem_off[:J], a.demods = doffs, _lib.ptr(dflat)
        _lib.check(_lib.lib().sdfr_decoder_styles(a, _lib.stream_of(lat)), "sdfr_decoder_styles")
        mods = [mflat[o:o + B * c].view(B, c) for o, c in zip(offs, self.mod_c)]
        demods = {i: dflat[o:o + B * c].view(B, c)
                  for i, o, c in zip(self.dem_layer, doffs, self.dem_c)}
        n = len(self.layers)
        return Styles(mods[:n], mods[n:], demods)

    def route(self, i, B, H, W, fuse_conv_act, fuse_conv_t_blur):
        """The launch layer ``i`` takes on a [B, H, W] input under the decoder's two fusion
        flags: ``"conv_act"`` (regular conv
        with the styled epilogue fused: the conv output stays on chip), ``"conv_t_act"``
        (upsampling conv with its blur and styled epilogue in the conv kernel: the same bits
        as the two launches), ``"split_conv+epilogue"`` or ``"miopen+epilogue"``.  The fused
        kernels write the split layout only, so they need a split-fp16 next layer."""
        ly = self.layers[i]
        if not ly.split:
            return "miopen+epilogue"
        last = i == len(self.layers) - 1
        if (fuse_conv_act and not ly.upsample and (last or self.layers[i + 1].split)
                and (H * W) % 256 == 0):
            return "conv_act"
        if (fuse_conv_t_blur and ly.upsample and not last and self.layers[i + 1].split
                and i % 2 == 1
                and _lib.lib().sdfr_conv_t_act_supported(B, H, W, ly.cin, ly.cout)):
            return "conv_t_act"
        return "split_conv+epilogue"


class FusedDecoder:
    """The fused HIP path of ``Decoder``.  It reads the decoder's modules and public flags
    (``use_fused``, ``conv_impl``, ``fuse_conv_act``, ``fuse_conv_t_blur``, ``conv_events``)
    and keeps no state but ``_plan`` and the event counter ``_conv_ev``."""

    def _plan_key(self):
        """One key for the whole plan: (data_ptr, version) of every tensor it derives data
        from -- an optimizer or EMA step, load_state_dict, .to() and deepcopy all change it
        -- and ``conv_impl``: (conv_impl, the weights' part, the blur kernels' part)."""
        return (self.conv_impl, *(tuple((t.data_ptr(), t._version) for t in ts)
                                  for ts in _plan_tensors(self)))

    def _fused_plan(self):
        """The plan of the current weights (rebuilt when the key changed)."""
        key = self._plan_key()
        if self._plan is None or self._plan.key != key:
            self._plan = DecoderPlan(self, key, self._plan)
        return self._plan

    def fused_ready(self, device, transform=None, rgbd_in=None):
        """Will forward() take the fused path for features on ``device``?  What depends on
        the decoder and the device only (checked before the features exist, so that
        prepare_fused can run beside the renderer)."""
        if not (self.use_fused and device.type == "cuda" and rgbd_in is None
                and transform is None):
            return False
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return False
        return self._fused_plan().supported

    def _fused_ok(self, features, rgbd_in, transform):
        if torch.is_grad_enabled() and features.requires_grad:
            return False
        return self.fused_ready(features.device, transform, rgbd_in)

    def prepare_fused(self, styles, B, device, noise=None, inject_index=None, truncation=1,
                      truncation_latent=None, input_is_latent=False, randomize_noise=True):
        """Everything of the fused forward that does not depend on the features: the
        mapping network, the noise maps and every layer's modulation / demodulation;
        forward(..., prepared=<this>) then runs the convolutions.  The same work, in
        the same order, as forward() does it."""
        latent, noise = self.styles_and_noise_forward(styles, noise, inject_index, truncation,
                                                      truncation_latent, input_is_latent,
                                                      randomize_noise)
        noise = self._fused_noise(noise, B, device, torch.float32)
        return Prepared(latent, noise, self._fused_plan().load().styles(latent))

    def _fused_noise(self, noise, B, device, dtype):
        """The per-layer noise maps of the fused path: the given ones, and every
        missing one (randomize_noise) sliced from ONE standard-normal draw of all of
        their elements, layer after layer -- one launch instead of one per layer (the
        module path draws each layer's map separately, NoiseInjection, so the two
        paths' random maps differ; their distribution does not)."""
        missing = [i for i, n in enumerate(noise) if n is None]
        if not missing:
            return noise
        sizes = [2 ** ((i + 2 * self.log_in_size + 1) // 2) for i in range(self.num_layers)]
        total = sum(B * sizes[i] * sizes[i] for i in missing)
        flat = torch.randn(total, device=device, dtype=dtype)
        out, off = list(noise), 0
        for i in missing:
            n = B * sizes[i] * sizes[i]
            out[i] = flat[off:off + n].view(B, 1, sizes[i], sizes[i])
            off += n
        return out

    def profile_convs(self, events):
        """Record `events[k] = (start, end)` around the k-th fused regular convolution of
        the next forward (None: stop); `conv_flops` counts their fp32-equivalent FLOPs."""
        self.conv_events, self._conv_ev, self.conv_flops = events, 0, 0

    @staticmethod
    def _fused_chunk(features, seq):
        """Faces per fused call: the largest activation of one face (a layer's input,
        or its raw output -- (2H+1) x (2W+1) for an upsampling layer -- in 4-byte
        elements) times the batch stays below 2^31 bytes (the 256^2 decoder: 63 faces)."""
        h, w = (features.shape[1:3] if features.dim() == 6 else features.shape[2:4])
        per_face = 0
        for sc in seq:
            cout, cin = sc.conv.weight.shape[1], sc.conv.weight.shape[2]
            per_face = max(per_face, h * w * cin * 4)
            if sc.conv.upsample:
                per_face = max(per_face, (2 * h + 1) * (2 * w + 1) * cout * 4)
                h, w = 2 * h, 2 * w
            per_face = max(per_face, h * w * cout * 4)
        return max(1, ((1 << 31) - 1) // per_face)

    @staticmethod
    def _noise_rows(noise, sl, B):
        """Faces ``sl`` of the per-layer noise maps: a [B, 1, h, w] map is sliced, a
        shared [1, 1, h, w] map (the decoder's fixed noise buffers) is kept."""
        return [n[sl] if n is not None and n.shape[0] == B else n for n in noise]

    def _fused_forward(self, features, latent, noise, sty=None):
        """Same computation as the module path: per layer one split-fp16 convolution
        (or MIOpen's) plus one sdfr_styled_epilogue on NHWC activations -- for the
        regular convolutions the epilogue runs inside the conv kernel
        (sdfr_conv3x3_f16x3_act); each activation is pre-multiplied by the next
        layer's modulation and the ToRGB layers are folded into the preceding
        epilogue."""
        cl = torch.channels_last
        B = features.shape[0]
        # (given styles are the current plan's: prepare_fused, or this call for a chunk)
        plan = self._plan if sty is not None else self._fused_plan().load()
        layers = plan.layers
        if sty is None:
            noise = self._fused_noise(noise, B, features.device, features.dtype)
            sty = plan.styles(latent)
        chunk = self._fused_chunk(features, plan.seq)
        if B > chunk:
            # the kernels index activations with 32-bit offsets (conv_launch: < 2^31 bytes
            # per tensor): larger batches run as chunks on the same noise maps and styles
            n_chunks = -(-B // chunk)
            chunk = -(-B // n_chunks)                     # balanced: 64 faces -> 2 x 32
            outs = []
            for b0 in range(0, B, chunk):
                sl = slice(b0, min(B, b0 + chunk))
                outs.append(self._fused_forward(features[sl], latent[sl],
                                                self._noise_rows(noise, sl, B), sty.rows(sl)))
            return torch.cat(outs, 0)
        mods, rgb_mods, demods = sty
        if features.dtype == torch.float16 and features.dim() == 6:
            # the renderer wrote features * mods[0] in the split layout already (ABI 12)
            if not layers[0].split:
                raise RuntimeError("decoder: split-NHWC features for a non-split first layer")
            x = features
            H, W = x.shape[1:3]
        else:
            x = (modulate_to_nhwc_split if layers[0].split else modulate_to_nhwc)(features,
                                                                                 mods[0])
            H, W = features.shape[2:4]
        rgb = None
        for i, ly in enumerate(layers):
            sc, mc = ly.sc, ly.sc.conv
            last = i == len(layers) - 1
            # this layer's part of the epilogue, whichever kernel runs it; a ToRGB's
            # modulated weight is base[o, c] * s[b, c] (the module path's weight * style)
            epi = dict(bias=sc.activate.bias, noise_weight=sc.noise.weight, noise=noise[i],
                       s_next=None if last else mods[i + 1])
            rgb_s = rgb_mods[i // 2] if ly.to_rgb is not None else None
            skip = rgb if i else None
            route = plan.route(i, B, H, W, self.fuse_conv_act, self.fuse_conv_t_blur)
            if route == "conv_act":
                # (events run out: later convolutions go unrecorded, not an IndexError)
                ev = self.conv_events if (self.conv_events is not None
                                          and self._conv_ev < len(self.conv_events)) else None
                if ev is not None:
                    ev[self._conv_ev][0].record()
                # the product base * s is formed inside the conv's epilogue (the same fp32
                # products, without a [B, 3, C] multiply launch)
                x, part = conv3x3_f16x3_act(x, ly.packed, ly.cout, demod=demods[i],
                                            store_y=not last, rgb_base=ly.rgb_base,
                                            rgb_s=rgb_s, **epi)
                if ev is not None:
                    ev[self._conv_ev][1].record()
                    self._conv_ev += 1
                    self.conv_flops += 2 * B * H * W * 9 * ly.cin * ly.cout
                if part is not None:
                    rgb = rgb_finish(part, ly.to_rgb.bias, skip=skip, fir=plan.fir)
            elif route == "conv_t_act":
                x = conv_t_act(x, ly.packed, ly.cout, fir=plan.fir, demod=demods[i], **epi)
            else:
                if route == "split_conv+epilogue":
                    out = conv3x3_f16x3(x, ly.packed, ly.cout, transposed=ly.upsample)
                    demod = demods[i]             # result carries su (power of two): exact
                else:
                    w = mc.scale * mc.weight[0]
                    demod = (torch.rsqrt((mods[i] * mods[i]) @ (w * w).sum([2, 3]).t() + 1e-8)
                             if mc.demodulate else None)
                    if ly.upsample:
                        out = F.conv_transpose2d(
                            x, w.transpose(0, 1).contiguous(memory_format=cl), stride=2)
                    else:
                        out = F.conv2d(x, w.contiguous(memory_format=cl), padding=mc.padding)
                rgb_w = rgb_b = None
                if ly.to_rgb is not None:
                    rgb_w, rgb_b = ly.rgb_base[None] * rgb_s[:, None, :], ly.to_rgb.bias
                x, rgb_new = styled_epilogue(
                    out, fir=plan.fir, demod=demod, blur_up=ly.upsample, store_y=not last,
                    rgb_w=rgb_w, rgb_b=rgb_b, skip=skip,
                    split_y=not last and layers[i + 1].split, **epi)
                if rgb_new is not None:
                    rgb = rgb_new
            if ly.upsample:
                H, W = 2 * H, 2 * W
        return rgb

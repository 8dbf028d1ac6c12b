"""TriPlaneGenerator: the object HFA-GP holds as ``self.generator``.

Drop-in surface: ``synthesis(ws, c, noise_mode='const') ->
{'image','image_raw','image_depth'}``, ``parameters()``, ``requires_grad_``,
``to()``, ``state_dict()`` with EG3D key names (``backbone.synthesis.b8.conv0.weight``
...), exactly what ``load_G_official`` (/root/reference/code/networks/headnerf.py:31-38)
hands to ``HeadNeRF_*`` and what ``trainer_rgb.py:59-60,70-71,143-151`` touch.

The arithmetic runs in libhfagp_hip.so (see ops.py).  There is no PyTorch
fallback: calling ``synthesis`` with CPU tensors or without the library raises.

The renderer's random draws (EG3D uses ``torch.rand_like`` / ``torch.rand``
inside ``ImportanceRenderer`` even in eval mode) are drawn here from the torch
device generator, or passed in as ``u_strat`` / ``u_imp`` for reproducible parity.
"""
from __future__ import annotations

import contextlib

import math
import os
from typing import Dict, Optional

import torch
from torch import nn

from . import ops, synthesis_call
from .config import GeneratorConfig, ffhq512_128


# --------------------------------------------------------------------------- parameter containers
class _Affine(nn.Module):
    def __init__(self, w_dim: int, cin: int, gen: torch.Generator):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cin, w_dim, generator=gen))
        self.bias = nn.Parameter(torch.ones(cin))           # bias_init = 1


class _SynthesisLayer(nn.Module):
    def __init__(self, cin, cout, w_dim, resolution, up, taps, gen, use_noise=True):
        super().__init__()
        self.up, self.resolution = up, resolution
        self.affine = _Affine(w_dim, cin, gen)
        self.weight = nn.Parameter(torch.randn(cout, cin, 3, 3, generator=gen))
        if use_noise:
            self.register_buffer("noise_const", torch.randn(resolution, resolution, generator=gen))
            self.noise_strength = nn.Parameter(torch.zeros([]))
        self.bias = nn.Parameter(torch.zeros(cout))
        self.register_buffer("resample_filter", _fir(taps))


class _ToRGB(nn.Module):
    def __init__(self, cin, cout, w_dim, gen):
        super().__init__()
        self.affine = _Affine(w_dim, cin, gen)
        self.weight = nn.Parameter(torch.randn(cout, cin, 1, 1, generator=gen))
        self.bias = nn.Parameter(torch.zeros(cout))


class _SynthesisBlock(nn.Module):
    def __init__(self, cin, cout, w_dim, resolution, img_channels, taps, gen):
        super().__init__()
        self.in_channels, self.out_channels, self.resolution = cin, cout, resolution
        if cin == 0:
            self.const = nn.Parameter(torch.randn(cout, resolution, resolution, generator=gen))
        else:
            self.conv0 = _SynthesisLayer(cin, cout, w_dim, resolution, 2, taps, gen)
        self.conv1 = _SynthesisLayer(cout, cout, w_dim, resolution, 1, taps, gen)
        self.torgb = _ToRGB(cout, img_channels, w_dim, gen)
        self.register_buffer("resample_filter", _fir(taps))


class _FC(nn.Module):
    def __init__(self, fin, fout, gen, lr_mul=1.0, bias_init=0.0):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(fout, fin, generator=gen) / lr_mul)
        self.bias = nn.Parameter(torch.full([fout], float(bias_init)))


# Above this many bytes of per-sample ray-marcher state (140 per sample: `ops.raymarch_state`) a differentiable step does not keep
# the state (the backward marches again) and `synthesis(normals=True)` renders in frame chunks.
RAY_STATE_CAP_BYTES = 8 << 30


def _fir(taps) -> torch.Tensor:
    k = torch.tensor(list(taps), dtype=torch.float32)
    k = torch.outer(k, k)
    return k / k.sum()


class _Synthesis(nn.Module):
    pass


class _Backbone(nn.Module):
    pass


class _Mapping(nn.Module):
    pass


class _SuperRes(nn.Module):
    pass


class _Decoder(nn.Module):
    pass


# --------------------------------------------------------------------------- the generator
class TriPlaneGenerator(nn.Module):
    def __init__(self, cfg: Optional[GeneratorConfig] = None, seed: int = 0):
        super().__init__()
        self.cfg = cfg = cfg or ffhq512_128()
        cfg.validate()
        if tuple(cfg.resample_filter) != (1, 3, 3, 1):
            raise ValueError("the fused up-sampling kernels are written for resample_filter [1,3,3,1]")
        gen = torch.Generator().manual_seed(seed)
        taps = cfg.resample_filter
        # EG3D attribute names (for state_dict compatibility)
        self.z_dim, self.c_dim, self.w_dim = cfg.z_dim, cfg.c_dim, cfg.w_dim
        self.img_resolution, self.img_channels = cfg.img_resolution, cfg.img_channels
        self.neural_rendering_resolution = cfg.neural_rendering_resolution

        self.backbone = _Backbone()
        syn = _Synthesis()
        for res in cfg.block_resolutions:
            cin = cfg.channels(res // 2) if res > 4 else 0
            setattr(syn, f"b{res}", _SynthesisBlock(cin, cfg.channels(res), cfg.w_dim, res,
                                                    cfg.backbone_img_channels, taps, gen))
        self.backbone.synthesis = syn
        mp = _Mapping()
        mp.embed = _FC(cfg.c_dim, cfg.w_dim, gen)
        for i in range(cfg.mapping_layers):
            setattr(mp, f"fc{i}", _FC(2 * cfg.w_dim if i == 0 else cfg.w_dim, cfg.w_dim, gen, cfg.mapping_lr_mul))
        mp.register_buffer("w_avg", torch.zeros(cfg.w_dim))
        self.backbone.mapping = mp

        sr = _SuperRes()
        r0, r1 = cfg.sr_resolutions
        sr.block0 = _SynthesisBlock(cfg.plane_channels, cfg.sr_channels[0], cfg.w_dim, r0, cfg.img_channels, taps, gen)
        sr.block1 = _SynthesisBlock(cfg.sr_channels[0], cfg.sr_channels[1], cfg.w_dim, r1, cfg.img_channels, taps, gen)
        self.superresolution = sr

        dec = _Decoder()
        dec.net = nn.ModuleDict({
            "0": _FC(cfg.plane_channels, cfg.decoder_hidden, gen, cfg.decoder_lr_mul),
            "2": _FC(cfg.decoder_hidden, 1 + cfg.plane_channels, gen, cfg.decoder_lr_mul),
        })
        self.decoder = dec
        self._prep: Dict[object, tuple] = {}     # (kind, ..., id(param)) -> (version, data_ptr, image, wsq)
        self._conv_precision = "fp32"
        self._sr_conv_precision: Optional[str] = None
        self.conv_precision = cfg.conv_precision
        self.sr_conv_precision = cfg.sr_conv_precision
        self.sr_storage = cfg.sr_storage
        # up-sampling layers in ONE pass (FIR fused into the transposed conv, csrc/upconv_fir.hip).  Measured on the MI355X
        # (profiles/r03_upfir/): the FIR arithmetic runs in the same waves as the GEMM, so the fused form only wins where the
        # GEMM is short and the layer is dominated by the round trip of the raw result through HBM — Cin <= 64, i.e. the first
        # super-resolution layer (32 -> 256 @128^2: 1.43 ms against 0.60 + 1.00 ms at B = 32); it ties or loses by 2 - 5 % on the
        # 256- and 512-channel layers.  "auto" (default): fused for Cin <= 64 where the launch fills the chip; "1": wherever the
        # library supports it; "0": never.
        self.fuse_up_fir = os.environ.get("HFAGP_FUSE_UP_FIR", "auto")
        # Image side chain (toRGB + skip of block k, and its adjoints) on a SECOND HIP stream for batches up to this value: same bits,
        # +1 % on one forward frame, two pathologies in fitting loops (allocator churn from record_stream marks; pool-stream aliasing
        # with collectives) — OFF by default (0); DESIGN.md section 8, round 4.
        self.side_stream_max_batch = int(os.environ.get("HFAGP_SIDE_STREAM_MAX_BATCH", "0"))
        self._side_streams: Dict[int, "torch.cuda.Stream"] = {}
        self._styles: Dict[int, tuple] = {}      # id(layer) -> (styles, dcoef) of the pass in flight
        self._absmax = None                      # (slot buffers, layer names) of the last pass: f16_range_report()
        self._rgb_part = None                    # partial toRGB sums of the conv just run (fused toRGB, ops.modconv)
        self._planes_absmax = None               # [64] slots with max |planes| of the pass in flight (16-bit decoder)
        self._scalars: Dict[int, tuple] = {}     # id(param) -> (version, data_ptr, python float)
        self._const_nhwc: Optional[tuple] = None
        self.timing: Optional[Dict[str, list]] = None   # bench.py: {'raymarch': [(ev0, ev1, units)], 'modconv': [...]}
        self.ignored_checkpoint_keys: list = []  # EG3D entries a loaded checkpoint carried that have no tensor here
        self._register_load_state_dict_pre_hook(self._drop_foreign_eg3d_keys)
        # a loaded checkpoint replaces parameters AND buffers in place: every derived image goes (the flat noise image)
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.invalidate_caches())

    # entries of an EG3D `G_ema.state_dict()` / HFA-GP `ckpt["gen"]["generator.*"]` that carry no parameter of the
    # path: version-dependent helper buffers of modules that are fused away here.  They are dropped (and listed in
    # `ignored_checkpoint_keys`) so that the reference's STRICT `load_state_dict` calls (trainer_rgb.py:137) succeed;
    # any other unexpected or missing key still raises.
    FOREIGN_KEY_PREFIXES = ("renderer.", "ray_sampler.", "superresolution.resample_filter")

    def _drop_foreign_eg3d_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                error_msgs):
        drop = [k for k in state_dict if k.startswith(prefix) and k[len(prefix):].startswith(self.FOREIGN_KEY_PREFIXES)]
        for k in drop:
            del state_dict[k]
        self.ignored_checkpoint_keys = [k[len(prefix):] for k in drop]

    def side_stream(self, batch: int, device) -> Optional["torch.cuda.Stream"]:
        """The second launch stream of `device` for the image side chain, or None when the batch is too large for it to pay
        (or while a HIP graph is being captured on the launch stream: a capture owns one stream)."""
        if batch > self.side_stream_max_batch or torch.cuda.is_current_stream_capturing():
            return None
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = self._side_streams.get(idx)
        if st is None:
            # from the HIGH-priority pool: PyTorch hands out its 32 default-priority pool streams round robin, and the collective
            # back ends take theirs from that same pool (gloo: one per asynchronous work) — a side stream from it ends up ALIASED
            # with a collective's copy stream every few steps and the image chain then queues behind host-side all-reduces
            # (measured: the 2-rank RGB fitting step 49 ms -> 2982 ms).  The high-priority pool is not used by them.
            st = self._side_streams[idx] = torch.cuda.Stream(device=device, priority=-1)
        return st

    def _timed(self, key: str, units: float, fn, *args, **kwargs):
        """Run ``fn`` bracketed by HIP events on the current stream when bench.py enabled timing."""
        if self.timing is None:
            return fn(*args, **kwargs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kwargs)
        e1.record()
        self.timing.setdefault(key, []).append((e0, e1, units))
        return out

    # ----------------------------------------------------------------- caches
    def invalidate_caches(self) -> None:
        """Drop every derived image of the parameters (GEMM weight images, wsq, host copies of scalars, the NHWC
        constant, the flat noise image).  The caches are keyed by (id, `_version`, `data_ptr`) of the parameter, which catches
        torch's own in-place ops, `load_state_dict` and `.to()` — and `MultiTensorAdam`, which bumps the versions itself; it does
        NOT catch `torch.optim.Adam(fused=True)` (leaves `_version` alone: the round-5 stale-image find) nor an in-place write through
        `.data` (EMA / PTI-style `.data.copy_`).  Hence: while any parameter requires grad every forward rebuilds the images
        (`_refresh_tuned`), the tuned -> frozen transition of the same object drops everything once, and callers that write through
        `.data` while frozen must call this.  Also called by `_apply` (device / dtype moves), `__deepcopy__` and after
        `load_state_dict` (post hook).  DESIGN.md section 5.2 lists every cache and its regression test."""
        self._prep = {}
        self._scalars = {}
        self._const_nhwc = None
        self._styles = {}
        self._plist = None
        self._conv_weights = None
        self._noise_layers = None
        self._noise_key = None
        self._scaled_noise = {}

    def _refresh_tuned(self, backward_follows: bool = True) -> None:
        """Start of every forward pass while ANY parameter requires grad (the generator is being tuned, trainer_rgb.py:69-71): drop the
        weight images / wsq / NHWC constant and re-read the 0-d parameters.  The caches are keyed by the parameters' `_version`, and an
        optimiser's in-place update does not reliably advance it: `torch.optim.Adam(fused=True)` — what the trainers build — moves
        every weight by lr per step and leaves `_version` at 0 (measured, round 5: rounds 2-4 ran the tuned step on the weight
        images of step 0, and timed it without the per-step image rebuild).  While the generator is frozen nothing here runs.
        The host copies of the noise strengths are refreshed in ONE device-to-host copy per step."""
        plist = getattr(self, "_plist", None)
        if plist is None:
            plist = self._plist = [p for n, p in self.named_parameters() if not n.startswith("backbone.mapping.")]
            self._scalar_params = [p for p in plist if p.dim() == 0]
        if not any(p.requires_grad for p in plist):
            self._scaled_noise = {}
            if getattr(self, "_was_tuned", False):
                # tuned -> frozen on the SAME object: what the last tuned forward cached predates the last optimiser step,
                # and the host copies of the noise strengths were never refreshed while tuned
                self._was_tuned = False
                self.invalidate_caches()
            return
        self._was_tuned = True
        self._prep = {}
        self._const_nhwc = None
        # noise strengths: NO host copy while tuned (a device-to-host read per step stalls the launch queue: +1.1 ms per step measured).
        # The forward kernels take noise_const * strength as their noise image with strength 1 (one gather + multiply over the 830 k
        # noise values of all layers), the fused backward pass reads the strength from device memory (noise_strength_dev).
        nl = getattr(self, "_noise_layers", None)
        # (the flat copy of the noise buffers follows them: load_state_dict / Trainer.resume copy into the buffers in place)
        nkey = None if nl is None else tuple((m.noise_const._version, m.noise_const.data_ptr()) for m in nl)
        if nl is None or nkey != getattr(self, "_noise_key", None):
            nl = self._noise_layers = [m for m in self.modules() if isinstance(m, _SynthesisLayer) and getattr(m, "noise_const", None) is not None]
            self._noise_key = tuple((m.noise_const._version, m.noise_const.data_ptr()) for m in nl)
            if nl:
                self._noise_flat = torch.cat([m.noise_const.detach().reshape(-1) for m in nl])
                self._noise_idx = torch.cat([torch.full((m.noise_const.numel(),), i, dtype=torch.long, device=self._noise_flat.device)
                                             for i, m in enumerate(nl)])
        self._scaled_noise = {}
        if nl:
            strengths = torch.stack([m.noise_strength.detach() for m in nl])
            scaled = self._noise_flat * strengths[self._noise_idx]
            off = 0
            for m in nl:
                n = m.noise_const.numel()
                self._scaled_noise[id(m)] = scaled[off: off + n].view_as(m.noise_const)
                off += n
        # ... and everything the step needs of the conv weights in ONE launch (ops.weight_prep_batch): forward image, image of the
        # transpose (when a backward pass can follow) and wsq; per-layer launches were 1.2 ms of a 15 ms step
        convs = getattr(self, "_conv_weights", None)
        if convs is None:
            convs = self._conv_weights = [(p, n.endswith((".conv0.weight", ".conv1.weight"))) for n, p in self.named_parameters()
                                          if n.endswith((".conv0.weight", ".conv1.weight", ".torgb.weight")) and p.dim() == 4]
        want_t = backward_follows        # (a call that records a tape: the bwd-data GEMMs will ask for the transposed images)
        items, owners = [], []
        for w, is_layer in convs:
            if not (w.is_cuda and ops.weight_prep_batch_supported(w)):
                continue
            prec, prec_t = self._precision_of(w), self._precision_of(w, True)
            prec = "f16x3" if prec == "f16x2" else prec
            prec_t = "f16x3" if prec_t == "f16x2" else prec_t
            if prec == "fp32":
                continue
            items.append((w.detach(), prec, prec_t if (want_t and prec_t != "fp32") else None, is_layer))
            owners.append((w, prec, prec_t))
        if items:
            for (w, prec, prec_t), (img, img_t, wsq) in zip(owners, ops.weight_prep_batch(items)):
                self._prep[("G", prec, False, id(w))] = (w._version, w.data_ptr(), img, None)
                if img_t is not None:
                    self._prep[("G", prec_t, True, id(w))] = (w._version, w.data_ptr(), img_t, None)
                if wsq is not None:
                    self._prep[("Q", id(w))] = (w._version, w.data_ptr(), None, wsq)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "_prep"):
            self.invalidate_caches()
        return out

    def __deepcopy__(self, memo):
        """`copy.deepcopy(generator)` (the reference's load_G_official deep-copies G_ema, headnerf.py:35): parameters,
        buffers and the precision settings are copied, the derived caches are not (their keys are object ids)."""
        import copy
        saved = (self._prep, self._scalars, self._const_nhwc, self._styles, self.timing)
        self.invalidate_caches()
        self.timing = None
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self._prep, self._scalars, self._const_nhwc, self._styles, self.timing = saved
        return new

    def _is_sr_weight(self, weight: torch.Tensor) -> bool:
        """True for the 3x3 conv weights of the two super-resolution blocks (resolved by module, not by a cached id)."""
        sr = self.superresolution
        return any(weight is l.weight for blk in (sr.block0, sr.block1) for l in (blk.conv0, blk.conv1))

    @property
    def conv_precision(self) -> str:
        """Arithmetic of the conv GEMMs: 'fp32' (exact MFMA), 'bf16x3' / 'bf16x6' / 'f16x3' (split-operand MFMA, fp32
        accumulation; include/hfagp.h HFAGP_PREC_*), 'f16' (single-pass fp16 MFMA, fp32 accumulation: the
        arithmetic of EG3D's fp16 blocks).  'f16x3' (the default) splits each operand into two fp16 parts (22 mantissa
        bits): fp32-class results at the cost of 'bf16x3'.  'f16x2' (opt-in): the 22-bit weights against activations rounded
        to ONE fp16 part, two MFMAs per product — the class of TF32, which the reference's cuDNN convs run in on Ampere-class
        GPUs (toRGB layers and gradient GEMMs stay as under 'f16x3').  Layers whose shape the 16-bit kernels do not take
        (Cin % 16, Cout % 128) always run on the exact fp32 kernel; gradient GEMMs of the fp16 kinds run in bf16x3 (a
        raw gradient has no place in fp16's exponent range without loss scaling)."""
        return self._conv_precision

    @property
    def sr_conv_precision(self) -> Optional[str]:
        """Precision of the super-resolution blocks' 3x3 convs; None = conv_precision."""
        return self._sr_conv_precision

    @sr_conv_precision.setter
    def sr_conv_precision(self, value: Optional[str]):
        if value is not None and value not in ops.PRECISIONS:
            raise ValueError(f"sr_conv_precision must be None or one of {sorted(ops.PRECISIONS)}, got {value!r}")
        self._sr_conv_precision = value

    @conv_precision.setter
    def conv_precision(self, value: str):
        if value not in ops.PRECISIONS:
            raise ValueError(f"conv_precision must be one of {sorted(ops.PRECISIONS)}, got {value!r}")
        self._conv_precision = value

    def _precision_of(self, weight: torch.Tensor, transposed: bool = False) -> str:
        """The precision a conv weight's GEMM runs in (the Cin/Cout transpose: the bwd-data GEMM)."""
        co, ci = weight.shape[:2]
        if transposed:
            co, ci = ci, co
        prec = self._conv_precision
        if self._sr_conv_precision is not None and self._is_sr_weight(weight):
            prec = self._sr_conv_precision
        if prec in ("f16", "f16x3", "f16x2") and transposed:
            prec = "bf16x3"       # gradient GEMMs: a raw gradient needs fp32's exponent range (bf16 parts have it)
        if prec in ("f16", "f16x2") and weight.shape[-1] == 1:
            prec = "f16x3"        # the toRGB products feed the tri-planes directly: keep them fp32-class
        if not ops.split_supported(ci, co):
            prec = "fp32"
        return prec

    def _gemm_image(self, weight: torch.Tensor, transposed: bool = False) -> torch.Tensor:
        """MFMA B-operand image of a conv weight (of its Cin/Cout transpose for the bwd-data GEMMs), in the layout
        of the configured precision; cached until the parameter changes."""
        prec = self._precision_of(weight, transposed)
        if prec == "f16x2":
            prec = "f16x3"        # same image: two fp16 parts of the weights (the ACTIVATIONS are the single part)
        key = ("G", prec, transposed, id(weight))
        hit = self._prep.get(key)
        if hit is not None and hit[0] == weight._version and hit[1] == weight.data_ptr():
            return hit[2]
        w = weight.detach()
        w = (w.transpose(0, 1) if transposed else w).contiguous()
        img = ops.weight_prep_prec(w, prec) if prec != "fp32" else ops.weight_prep(w)[0]
        self._prep[key] = (weight._version, weight.data_ptr(), img, None)
        return img

    def _prepared(self, weight: torch.Tensor):
        """(GEMM image, wsq [Cout, Cin] = sum over taps of weight^2 for the demodulation)."""
        key = ("Q", id(weight))
        hit = self._prep.get(key)
        if hit is None or hit[0] != weight._version or hit[1] != weight.data_ptr():
            _, wsq = ops.weight_prep(weight.detach().contiguous())
            hit = (weight._version, weight.data_ptr(), None, wsq)
            self._prep[key] = hit
        return self._gemm_image(weight), hit[3]

    def _scalar(self, t: torch.Tensor) -> float:
        """Host copy of a 0-d parameter (noise_strength), cached so steady state has no device sync."""
        hit = self._scalars.get(id(t))
        if hit is not None and hit[0] == t._version and hit[1] == t.data_ptr():
            return hit[2]
        v = float(t.detach())
        self._scalars[id(t)] = (t._version, t.data_ptr(), v)
        return v

    def _const(self, const: torch.Tensor) -> torch.Tensor:
        hit = self._const_nhwc
        if hit is not None and hit[0] == const._version and hit[1] == const.data_ptr():
            return hit[2]
        x = ops.nchw_to_nhwc(const.detach()[None].contiguous())
        self._const_nhwc = (const._version, const.data_ptr(), x)
        return x

    # ----------------------------------------------------------------- layers
    def _layer(self, x, layer: _SynthesisLayer, w, row, batch, noise_mode, conv_clamp, tape, x_absmax=None,
               y_absmax=None, rgb=None, half=False, keep_out=True):
        """x_absmax / y_absmax: fp16 range tracking of an UNCLAMPED activation chain (ops.modconv): the slot buffer with
        max |x| of the input as published by its producer, and the one this layer publishes max |out| into.
        half: write the output (and the raw up-conv intermediate) as float16 (`sr_storage = "f16"`, no tape)."""
        cfg = self.cfg
        wt, wsq = self._prepared(layer.weight)
        pre = self._styles.pop(id(layer), None) if self._styles else None      # computed up front (_precompute_styles)
        styles, dcoef = pre if pre is not None else ops.styles_demod(w, layer.affine.weight, layer.affine.bias, wsq,
                                                                     1.0, cfg.demod_eps)
        noise, ns = None, 0.0
        noise_raw, ns_dev = None, None
        if noise_mode == "const":
            scaled = getattr(self, "_scaled_noise", {}).get(id(layer))
            if scaled is not None:       # generator being tuned (_refresh_tuned): pre-scaled noise image, strength stays on the device
                noise, ns, noise_raw, ns_dev = scaled, 1.0, layer.noise_const, layer.noise_strength.detach()
            else:
                noise, ns = layer.noise_const, self._scalar(layer.noise_strength)
                noise_raw = noise
        elif noise_mode != "none":
            raise NotImplementedError("noise_mode must be 'const' or 'none' (HFA-GP passes 'const', headnerf.py:112)")
        cout = layer.weight.shape[0]
        gain = math.sqrt(2.0)
        x_parts = 1 if self._precision_of(layer.weight) == "f16x2" else 0
        k_styles, k_dcoef = styles, dcoef       # (the fp16 kernels apply EG3D's fp16 range guard themselves)
        # algorithmic FLOPs: 2 * B * H_in * W_in * Cin * Cout * 9 (the up-conv is counted in its
        # polyphase / transposed form at INPUT resolution)
        flops = 2.0 * batch * x.shape[1] * x.shape[2] * x.shape[3] * cout * 9
        # which kernel bench.py times
        key = ("modconv" if wt.dtype == torch.float32 else
               "modconv_f16" if wt.dtype == torch.float16 and wt.shape[0] == 1 else "modconv_split")
        npos = x.shape[1] * x.shape[2]
        if (layer.up != 2 and wt.dtype != torch.float32 and npos <= 256 and x.shape[3] % 16 == 0
                and x.shape[3] <= 512 and cout % 32 == 0 and not half and rgb is None
                and not (npos >= 64 and batch * npos >= 1024)):     # (the batch term of the predicate: staged kernel from 1024 positions)
            # the library runs these on smallconv_kernel (csrc/smallconv.hip, modconv_plan.h `smallconv_takes` — same predicate:
            # fp16-storage, Cin > 512 and fused-toRGB layers stay on the staged kernel): not the roofline kernel
            key = "modconv_small"
        fuse = self.fuse_up_fir
        # (fp16 STORAGE halves the stand-alone FIR kernel's traffic: there the two-kernel form measured 0.6 % ahead)
        fuse = fuse in (True, "1") or (fuse == "auto" and x.shape[3] <= 64 and not half)
        if layer.up == 2 and fuse and ops.upconv_fir_supported(x, wt, cout, batch):
            # the whole up-sampling layer in one pass: the raw transposed-conv result stays on the chip (csrc/upconv_fir.hip)
            def fused_layer():
                return self._timed(key + "_upfir", flops, ops.upconv_fir, x, wt, cout, k_styles, k_dcoef, noise, ns, layer.bias,
                                   "lrelu", cfg.lrelu_alpha, gain, conv_clamp, batch=batch, x_absmax=x_absmax,
                                   y_absmax=y_absmax, y_f16=half)
            out = self._timed(f"up_layer:{x.shape[3]}->{cout}@{2 * x.shape[1]}:fused", flops, fused_layer)
        elif layer.up == 2:
            def two_kernels():
                yt = self._timed(key + "_up", flops, ops.modconv, x, wt, cout, ops.CONVT3X3_UP2, styles=k_styles, batch=batch,
                                 x_absmax=x_absmax, y_f16=half, x_parts=x_parts)
                return ops.upfir_epilogue(yt, k_dcoef, noise, ns, layer.bias, "lrelu", cfg.lrelu_alpha, gain, conv_clamp,
                                          y_absmax=y_absmax)
            # (bench.py `roofline.up_layers`: the LAYER — transposed-conv GEMM + FIR epilogue — per shape)
            out = self._timed(f"up_layer:{x.shape[3]}->{cout}@{2 * x.shape[1]}", flops, two_kernels)
        else:
            # rgb = (toRGB weight [3, Cout], toRGB styles [B, Cout]): form the block's toRGB sums in this conv's epilogue
            # when the kernel can (ops.fused_torgb_supported); the caller finishes them with ops.torgb_finish
            rgb_w = None
            if rgb is not None and ops.fused_torgb_supported(x, wt, cout, batch):
                rgb_w = (rgb[1][:, None, :] * rgb[0][None]).contiguous()
            out = self._timed(key, flops, ops.modconv, x, wt, cout, ops.CONV3X3, styles=k_styles, dcoef=k_dcoef,
                              noise=noise, noise_strength=ns, bias=layer.bias, act="lrelu", alpha=cfg.lrelu_alpha,
                              gain=gain, clamp=conv_clamp, batch=batch, x_absmax=x_absmax, y_absmax=y_absmax,
                              rgb_w=rgb_w, y_f16=half, x_parts=x_parts,
                              store_y=keep_out or rgb_w is None or tape is not None or y_absmax is not None)
            if rgb_w is not None:
                out, self._rgb_part = out
        rec = None
        if tape is not None:
            rec = dict(layer=layer, x=x, styles=styles, dcoef=dcoef, out=out, row=row, up=layer.up, wsq=wsq,
                       producer=dict(dcoef=dcoef, bias=layer.bias, noise=noise_raw, noise_strength=ns if ns_dev is None else 0.0,
                                     noise_strength_dev=ns_dev, act="lrelu", alpha=cfg.lrelu_alpha, gain=gain, clamp=conv_clamp))
        return out, rec

    def _block(self, x, img, blk: _SynthesisBlock, ws, rows, batch, noise_mode, conv_clamp, small_rgb, last, tape,
               absmax=None, half=False, keep_out=True):
        """keep_out=False: nobody reads this block's feature output x (the last super-resolution block): when its toRGB
        rides in conv1's epilogue and nothing is recorded for a backward pass, conv1 does not store its activation (x is
        then returned as None).
        rows = the ws row of (conv0,) conv1, torgb.  absmax = (slots of the block input | None, slots for conv0's
        output, slots for conv1's output) when the chain is unclamped (fp16 range tracking), else None."""
        rec = dict(conv0=None, first=blk.in_channels == 0, img_in=img, const=getattr(blk, "const", None))
        am_in, am0, am1 = absmax if absmax is not None else (None, None, None)
        tr = blk.torgb
        cin = tr.weight.shape[1]
        row = rows[-1]
        pre = self._styles.pop(id(tr), None) if self._styles else None
        styles = pre[0] if pre is not None else ops.styles_demod(ws[:, row], tr.affine.weight, tr.affine.bias, None,
                                                                 1.0 / math.sqrt(cin))[0]
        # a 3-channel toRGB (super-resolution blocks) rides in the epilogue of conv1 where the kernel allows it
        rgb = (tr.weight.detach().reshape(tr.weight.shape[0], cin), styles) if (small_rgb and tr.weight.shape[0] <= 3) else None
        self._rgb_part = None
        if blk.in_channels == 0:
            x, rec["conv1"] = self._layer(self._const(blk.const), blk.conv1, ws[:, rows[0]], rows[0], batch,
                                          noise_mode, conv_clamp, tape, None, am1, rgb)
        else:
            x, rec["conv0"] = self._layer(x, blk.conv0, ws[:, rows[0]], rows[0], batch, noise_mode, conv_clamp, tape,
                                          am_in, am0, None, half)
            x, rec["conv1"] = self._layer(x, blk.conv1, ws[:, rows[1]], rows[1], batch, noise_mode, conv_clamp, tape,
                                          am0, am1, rgb, half, keep_out)
        y = y_pre = None
        if small_rgb:
            if tape is not None and conv_clamp is not None:
                y_pre = torch.empty(batch, tr.weight.shape[0], x.shape[1], x.shape[2], device=x.device)
            if self._rgb_part is not None:
                img = ops.torgb_finish(self._rgb_part, tr.bias, img, conv_clamp, y_pre)
                self._rgb_part = None
            else:
                img = ops.torgb_small(x.float() if half else x, tr.weight.detach().reshape(tr.weight.shape[0], cin),
                                      styles, tr.bias, img, conv_clamp, y_pre)
        else:
            wt = self._gemm_image(tr.weight)          # (no demodulation: no wsq)
            side = self.side_stream(batch, x.device)
            main = torch.cuda.current_stream(x.device) if side is not None else None
            if side is not None:
                side.wait_stream(main)               # conv1's output (and everything before it) is ordered before the side chain
                for t in (x, styles):                # main-stream tensors read on the side stream: not to be recycled under it
                    t.record_stream(side)
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                # the block that writes the tri-planes also publishes max |planes|: the bound the ray marcher's 16-bit
                # decoder scales its operands by (ops.raymarch planes_absmax)
                self._planes_absmax = ops.absmax_slots(1, x.device)[0] if last else None
                if conv_clamp is None and x.shape[0] == batch and ops.torgb_skip_supported(x, wt, tr.weight.shape[0]):
                    # toRGB and the skip connection in one streaming pass (the toRGB output is never stored)
                    img = ops.torgb_skip(x, wt, tr.weight.shape[0], styles, tr.bias, img, plane_major=last, x_absmax=am1,
                                         out_absmax=self._planes_absmax)
                else:
                    y = ops.modconv(x, wt, tr.weight.shape[0], ops.CONV1X1, styles=styles, bias=tr.bias, act="linear",
                                    gain=1.0, clamp=conv_clamp, batch=batch, x_absmax=am1)
                    img = ops.skip_upsample_add(img, y, plane_major=last, out_absmax=self._planes_absmax)
            if side is not None and last:
                # join: the tri-planes (and their |max| slots) are consumed on the launch stream from here on
                main.wait_stream(side)
                img.record_stream(main)
                self._planes_absmax.record_stream(main)
        if tape is not None:
            rec["rgb"] = dict(torgb=tr, x=x, styles=styles, row=row, small=small_rgb, clamp=conv_clamp,
                              y=y if conv_clamp is not None else None, y_pre=y_pre)
            tape.append(rec)
        return x, img

    def _precompute_styles(self, ws: torch.Tensor, blocks_rows) -> None:
        """Styles (and demodulation coefficients) of every layer of ``blocks_rows`` = [(block, rows)] in two
        launches; `_layer` / `_block` pick them up by layer identity."""
        cfg = self.cfg
        items, keys = [], []
        for blk, rows in blocks_rows:
            convs = [blk.conv1] if blk.in_channels == 0 else [blk.conv0, blk.conv1]
            for layer, row in zip(convs, rows):
                items.append((ws[:, row], layer.affine.weight, layer.affine.bias, self._prepared(layer.weight)[1], 1.0,
                              cfg.demod_eps))
                keys.append(id(layer))
            tr = blk.torgb
            items.append((ws[:, rows[-1]], tr.affine.weight, tr.affine.bias, None, 1.0 / math.sqrt(tr.weight.shape[1]),
                          cfg.demod_eps))
            keys.append(id(tr))
        self._styles = {}
        for i in range(0, len(items), 32):
            for k, v in zip(keys[i:i + 32], ops.styles_demod_batch(items[i:i + 32])):
                self._styles[k] = v

    # ----------------------------------------------------------------- public API
    def backbone_planes(self, ws: torch.Tensor, tape=None) -> torch.Tensor:
        """ws [B, num_ws, 512] → tri-plane volume [B, 3, R, R, 32] (plane-major, channels-last)."""
        if not getattr(self, "_in_forward", False):     # called directly (not through synthesis): the derived images follow the weights
            self._refresh_tuned(tape is not None)
        cfg = self.cfg
        syn = self.backbone.synthesis
        b = ws.shape[0]
        x = img = None
        idx = 0
        plan = []
        for res in cfg.block_resolutions:
            n_conv = 1 if res == 4 else 2
            plan.append((getattr(syn, f"b{res}"), list(range(idx, idx + n_conv + 1))))
            idx += n_conv
        self._precompute_styles(ws, plan)
        # fp16 range tracking: the backbone has no clamp (conv_clamp None), so every conv publishes max |out| and the
        # next fp16-kind GEMM normalises its operand with it (one memset for all layers; row 2k / 2k+1 = conv0 / conv1
        # of block k).  Kept for `f16_range_report()`.
        track = cfg.backbone_conv_clamp is None and (self._conv_precision in ("f16x3", "f16x2", "f16"))
        am = ops.absmax_slots(2 * len(cfg.block_resolutions), ws.device) if track else None
        self._absmax = (am, [f"b{res}.{c}" for res in cfg.block_resolutions for c in ("conv0", "conv1")]) if track else None
        idx = 0
        prev = None
        for k, res in enumerate(cfg.block_resolutions):
            blk = getattr(syn, f"b{res}")
            n_conv = 1 if res == 4 else 2
            rows = list(range(idx, idx + n_conv + 1))
            x, img = self._block(x, img, blk, ws, rows, b, cfg.backbone_noise_mode, cfg.backbone_conv_clamp, False,
                                 res == cfg.plane_resolution, tape,
                                 (prev, am[2 * k], am[2 * k + 1]) if track else None)
            prev = am[2 * k + 1] if track else None
            idx += n_conv
        side = self._side_streams.get(ws.device.index if ws.device.index is not None else torch.cuda.current_device())
        if side is not None and not torch.cuda.is_current_stream_capturing():
            # join of the image side chain, whatever block ended it (not inside a HIP-graph capture: side_stream() declines there,
            # and waiting on a stream outside the capture would invalidate it — ADVICE r4)
            torch.cuda.current_stream(ws.device).wait_stream(side)
        return img

    def f16_range_report(self) -> Optional[Dict[str, float]]:
        """max |activation| of every backbone layer output of the LAST synthesis (host sync), or None when the conv
        precision has no fp16 parts / the backbone is clamped.  Values beyond 65504 are handled (the consumer GEMM
        scales by an exact power of two, hfagp.h `x_absmax`); the report shows how far a checkpoint is from the cliff
        that an un-tracked fp16 split would have."""
        if getattr(self, "_absmax", None) is None:
            return None
        am, names = self._absmax
        vals = am.max(dim=1).values.tolist()
        return {n: v for n, v in zip(names, vals) if not n.startswith("b4.conv0")}

    def decoder_params(self):
        """The decoder's parameters in the order of the ops' dec_w0, dec_b0, dec_w1, dec_b1."""
        net = self.decoder.net
        return net["0"].weight, net["0"].bias, net["2"].weight, net["2"].bias

    def _render_args(self, c: torch.Tensor, res: Optional[int] = None):
        """`res`: the ray resolution of the call (a backward pass hands in its forward's); None = the current one."""
        cfg = self.cfg
        hit = getattr(self, "_cam_cache", None)       # the backward pass of a step asks again with the forward's tensor
        if hit is None or hit[0] is not c or hit[1] != c._version:
            hit = self._cam_cache = (c, c._version, c[:, :16].contiguous(), c[:, 16:25].contiguous())
        return dict(zip(ops._DEC, self.decoder_params()), cam2world=hit[2], intrinsics=hit[3],
                    res=self.neural_rendering_resolution if res is None else res, ray_start=cfg.ray_start, ray_end=cfg.ray_end,
                    box_warp=cfg.box_warp, decoder_lr_mul=cfg.decoder_lr_mul,
                    plane_axes=ops._plane_axes_id(cfg.plane_axes), white_back=cfg.white_back,
                    decoder_precision=cfg.decoder_precision)

    def _uniforms(self, b: int, dev, u_strat, u_imp):
        cfg = self.cfg
        r = self.neural_rendering_resolution ** 2
        if u_strat is None:
            u_strat = torch.rand(b, r, cfg.depth_resolution, device=dev)
        if u_imp is None:
            u_imp = torch.rand(b * r, cfg.depth_resolution_importance, device=dev)
        return u_strat.reshape(b, r, -1).contiguous(), u_imp.contiguous()

    def render(self, planes: torch.Tensor, c: torch.Tensor, u_strat=None, u_imp=None, planes_absmax=None, state=None):
        """state (ops.raymarch_state): filled with the per-sample results the backward pass of this step will need."""
        cfg = self.cfg
        b = planes.shape[0]
        r = self.neural_rendering_resolution ** 2
        u_strat, u_imp = self._uniforms(b, planes.device, u_strat, u_imp)
        # algorithmic bytes per frame: samples * 3 planes * 4 taps * 32 ch * 4 B
        # + outputs R*(32+1+1)*4 + uniforms R*(Sc+Sf)*4
        s_tot = cfg.depth_resolution + cfg.depth_resolution_importance
        nbytes = float(b) * r * (s_tot * 3 * 4 * 32 * 4 + 34 * 4 + s_tot * 4)
        return self._timed("raymarch", nbytes, ops.raymarch, planes, u_strat=u_strat, u_imp=u_imp,
                           planes_absmax=planes_absmax, state=state, **self._render_args(c))

    def _render_normals_chunked(self, planes, c, u_strat, u_imp, planes_absmax, frames: int):
        """`render` + `ops.raymarch_normals` over chunks of `frames` frames through one state buffer of that size: the per-sample
        state of the whole batch would exceed RAY_STATE_CAP_BYTES.  Every ray is computed as in the whole-batch launch (the
        decoder's bound on |planes| is the batch's, taken once), so the five results equal the unchunked ones bit for bit."""
        cfg = self.cfg
        b, res = planes.shape[0], self.neural_rendering_resolution
        planes_absmax = ops._decoder_bound(planes, cfg.decoder_precision, planes_absmax)
        u_imp = u_imp.view(b, res * res, -1)
        state = ops.raymarch_state(min(frames, b), res, cfg.depth_resolution, cfg.depth_resolution_importance, planes.device)
        parts = []
        for i in range(0, b, frames):
            n = min(frames, b - i)
            pl, ci, us, ui = planes[i:i + n], c[i:i + n], u_strat[i:i + n], u_imp[i:i + n].reshape(n * res * res, -1)
            out = self.render(pl, ci, us, ui, planes_absmax=planes_absmax, state=state[:n])
            parts.append(out + (ops.raymarch_normals(pl, state[:n], u_strat=us, u_imp=ui, planes_absmax=planes_absmax,
                                                     **self._render_args(ci)),))
        return tuple(torch.cat(t) for t in zip(*parts))

    def superres(self, rgb_raw: torch.Tensor, feat_img: torch.Tensor, ws: torch.Tensor, tape=None) -> torch.Tensor:
        if not getattr(self, "_in_forward", False):     # called directly: see backbone_planes
            self._refresh_tuned(tape is not None)
        cfg = self.cfg
        b = ws.shape[0]
        last = cfg.num_ws - 1
        sr = self.superresolution
        self._precompute_styles(ws, [(sr.block0, [last] * 3), (sr.block1, [last] * 3)])
        half = self._sr_half(b, feat_img.shape[1], tape)
        x, rgb = self._block(feat_img, rgb_raw, sr.block0, ws, [last] * 3, b, cfg.sr_noise_mode, cfg.sr_conv_clamp,
                             True, False, tape, None, half)
        x, rgb = self._block(x, rgb, sr.block1, ws, [last] * 3, b, cfg.sr_noise_mode, cfg.sr_conv_clamp, True, False,
                             tape, None, half, keep_out=False)
        return rgb

    def _sr_half(self, batch: int, res: int, tape) -> bool:
        """fp16 STORAGE of the super-resolution activations (cfg.sr_storage = "f16"): EG3D's own arrangement for these two
        blocks (sr_num_fp16_res = 4: fp16 tensors between the layers, clamp 256).  Taken only where the arithmetic is
        the single-pass fp16 one (sr_conv_precision "f16"), nothing is recorded for a backward pass, and every conv of
        the two blocks is one the kernels can run that way (ops.f16_storage_supported)."""
        cfg = self.cfg
        if self.sr_storage != "f16" or self._sr_conv_precision != "f16" or tape is not None:
            return False
        if cfg.sr_conv_clamp is None:
            return False                  # fp16 storage relies on the clamp (|x| <= 256) for its range
        c0, c1 = cfg.sr_channels
        ok = ops.f16_storage_supported
        return (ok(res, res, cfg.plane_channels, c0, batch) and ok(2 * res, 2 * res, c0, c0, batch) and
                ok(2 * res, 2 * res, c0, c1, batch) and ok(4 * res, 4 * res, c1, c1, batch))

    def _check_inputs(self, ws, c, noise_mode):
        cfg = self.cfg
        if not ws.is_cuda:
            raise RuntimeError("TriPlaneGenerator.synthesis: the MI355X path needs CUDA/ROCm tensors; "
                               "there is no CPU fallback (oracle/ is test infrastructure only)")
        if noise_mode != "const":
            raise NotImplementedError("HFA-GP always passes noise_mode='const' (headnerf.py:112)")
        if ws.device.index != torch.cuda.current_device():
            raise RuntimeError(f"TriPlaneGenerator.synthesis: tensors live on {ws.device} but the current device is "
                               f"cuda:{torch.cuda.current_device()}; the kernels are enqueued on the CURRENT device's "
                               f"stream — wrap the call in `with torch.cuda.device(ws.device):`")
        if c.dim() not in (2, 3):
            raise ValueError(f"expected c [B,{cfg.c_dim}] (one camera per latent) or [B,V,{cfg.c_dim}] (V views of every latent), got "
                             f"{tuple(c.shape)}")
        if ws.shape[1:] != (cfg.num_ws, cfg.w_dim) or c.shape[-1] != cfg.c_dim or (c.dim() == 3 and c.shape[0] != ws.shape[0]):
            raise ValueError(f"expected ws [B,{cfg.num_ws},{cfg.w_dim}] and c [B,{cfg.c_dim}] or [B,V,{cfg.c_dim}], got "
                             f"{tuple(ws.shape)} and {tuple(c.shape)}")

    def _set_resolution(self, b: int, n: Optional[int], u_strat, u_imp) -> None:
        """`synthesis(neural_rendering_resolution=n)`: validates and stores the ray resolution of this and later calls (None: the
        stored one), and checks caller-given uniforms against it."""
        cfg = self.cfg
        r0 = cfg.neural_rendering_resolution
        if n is None:
            n = self.neural_rendering_resolution
        elif isinstance(n, bool) or int(n) != n or not (r0 <= 4 * n and n <= 4 * r0):
            raise ValueError(f"TriPlaneGenerator.synthesis: neural_rendering_resolution={n!r} must be an integer in "
                             f"[{-(-r0 // 4)}, {4 * r0}] (a quarter to four times the configured {r0})")
        for name, u, s in (("u_strat", u_strat, cfg.depth_resolution), ("u_imp", u_imp, cfg.depth_resolution_importance)):
            if u is not None and u.numel() != b * n * n * s:
                raise ValueError(f"TriPlaneGenerator.synthesis: {name} {tuple(u.shape)} is not sized for {n}^2 rays of {s} samples "
                                 f"in {b} frames")
        self.neural_rendering_resolution = int(n)

    def _check_normal_grad(self, ws, c, normal_camera_grad: bool = False) -> None:
        """The refusals of `synthesis(normal_grad=True)` under grad, before anything is launched."""
        cfg = self.cfg
        if c.requires_grad and not normal_camera_grad:
            raise NotImplementedError("TriPlaneGenerator.synthesis(normal_grad=True): the camera gradient of the normal term is opt-in "
                                      "(c.requires_grad): pass normal_camera_grad=True for it, detach the label, or use normals=True "
                                      "for a detached map")
        frames = c.numel() // cfg.c_dim          # B, or B·V of a multi-view label
        frame_bytes = self.neural_rendering_resolution ** 2 * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
        if frames * frame_bytes > RAY_STATE_CAP_BYTES:
            raise RuntimeError(f"TriPlaneGenerator.synthesis(normal_grad=True): the backward of 'image_normal' reads the ray marcher's "
                               f"per-sample state, {frames * frame_bytes} bytes for {frames} frames, above "
                               f"RAY_STATE_CAP_BYTES = {RAY_STATE_CAP_BYTES}; {RAY_STATE_CAP_BYTES // frame_bytes} frames fit")

    def _forward_impl(self, call, ws, c, tape):
        """The one forward of `synthesis`, under no_grad.  call: the synthesis_call.SynthesisCall; ws, c: detached contiguous fp32
        CUDA tensors.  Returns image, image_raw, image_depth, image_mask, query_sigma, query_rgb, query_sigma_grad, query_normal,
        image_normal — None for what the call did not ask for — and leaves the planes and the feature image in the record; when
        `tape` is a dict it is filled with everything the backward pass needs."""
        self._refresh_tuned(tape is not None)
        self._in_forward = True          # (backbone_planes / superres below must not rebuild the images a second time)
        try:
            img, rgb_raw, depth, mask, normal, call.planes, call.feature_image = self._forward_body(
                ws, c, call.u_strat, call.u_imp, tape, call.geometry, call.normals, call.views)
        finally:
            self._in_forward = False
        q = {}
        pam = getattr(self, "_planes_absmax", None)
        if call.query is not None and call.query_normals:        # the same launch slot, four outputs
            q = self._timed("planes_query_normals", float(ws.shape[0]), ops.planes_query_normals, call.planes, call.query,
                            planes_absmax=pam, **self._query_kwargs())
        elif call.query is not None:            # points evaluated on this call's planes
            q["sigma"], q["rgb"] = ops.planes_query(call.planes, call.query, planes_absmax=pam, **self._query_kwargs())
        return img, rgb_raw, depth, mask, q.get("sigma"), q.get("rgb"), q.get("grad"), q.get("normal"), normal

    @staticmethod
    def _per_frame(t: torch.Tensor, views: Optional[int]) -> torch.Tensor:
        """A per-identity tensor [B, ...] as the per-frame one [B·V, ...] of a multi-view call, frame b·V + v reading identity b: a copy
        (V > 1), or `t` itself (a single-view call, and V = 1)."""
        if views is None or views == 1:
            return t
        # (.contiguous(): at B = 1 the reshape alone is still the stride-0 view)
        return t[:, None].expand(-1, views, *t.shape[1:]).reshape(-1, *t.shape[1:]).contiguous()

    def _forward_body(self, ws, c, u_strat, u_imp, tape, geometry, normals, views=None):
        """→ image, image_raw, depth, the opacity image [F,1,r,r] (`geometry`; else None), 'image_normal' (`normals`: the same
        per-sample results feed the normal pass; else None), planes, feat_img.  `views` = V of a multi-view call (c is then the
        flattened label [B·V, 25]): the backbone runs at batch B, everything from the planes on at F = B·V frames, frame b·V + v on
        the planes and the ws rows of identity b; every result but `planes` [B] is per frame.  None: F = B."""
        cfg = self.cfg
        ids = ws.shape[0]
        res, res_sr = self.neural_rendering_resolution, cfg.neural_rendering_resolution      # rays marched; the SR blocks' input
        bb_tape = [] if tape is not None else None
        sr_tape = [] if tape is not None else None
        planes_id = self.backbone_planes(ws, bb_tape)
        # the renderer's kernels index the planes by frame: the V frames of an identity read a transient copy of its planes (V·|planes|
        # bytes, 25 MB per frame at 256² — a ninth of a frame's ray state); the tape keeps the identity's one set
        planes, ws = self._per_frame(planes_id, views), self._per_frame(ws, views)
        b = ids if views is None else ids * views
        u_strat, u_imp = self._uniforms(b, ws.device, u_strat, u_imp)
        pam = getattr(self, "_planes_absmax", None)
        # a step that will be differentiated keeps the ray marcher's per-sample results (220 MB per frame at 128^2 rays x 96
        # samples; skipped above 8 GB): the compositing adjoint then reads them instead of marching every ray again
        ray_state = normal = None
        frame_bytes = res * res * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
        if (tape is not None or normals) and b * frame_bytes <= RAY_STATE_CAP_BYTES:
            ray_state = ops.raymarch_state(b, res, cfg.depth_resolution, cfg.depth_resolution_importance, ws.device)
        if normals and ray_state is None:         # above the cap: render and take the normals in frame chunks
            feat, depth, wsum, tmm, normal = self._render_normals_chunked(planes, c, u_strat, u_imp, pam,
                                                                          max(1, RAY_STATE_CAP_BYTES // frame_bytes))
        else:
            feat, depth, wsum, tmm = self.render(planes, c, u_strat, u_imp, planes_absmax=pam, state=ray_state)
            if normals:
                normal = ops.raymarch_normals(planes, ray_state, u_strat=u_strat, u_imp=u_imp, planes_absmax=pam,
                                              **self._render_args(c))
        if normals:
            normal = normal.view(b, res, res, 3).permute(0, 3, 1, 2).contiguous()      # NCHW, 'image_normal'
            if tape is None:
                ray_state = None                  # (not needed again: released before the super-resolution allocates)
        del planes                                # (so is a multi-view call's per-frame copy)
        # MipRayMarcher2 clamps the expected depth to the GLOBAL min/max sample depth of the batch
        depth = ops.depth_clamp_(depth, tmm)
        feat_img = feat.view(b, res, res, 32)                             # channels-last
        rgb_raw = feat_img[..., :3].permute(0, 3, 1, 2).contiguous()      # NCHW, 'image_raw'
        feat_sr, rgb_sr = feat_img, rgb_raw
        if res != res_sr:
            # SuperresolutionHybrid8XDC.forward brings rgb and x back to its input resolution (antialiased bilinear); per channel, so
            # one pass over the feature image serves both
            feat_sr = self._timed("resize_aa", float(b) * (res * res + res_sr * res_sr) * 128, ops.resize_aa, feat_img, (res_sr, res_sr))
            rgb_sr = feat_sr[..., :3].permute(0, 3, 1, 2).contiguous()
        img = self.superres(rgb_sr, feat_sr, ws, sr_tape)
        if tape is not None:
            # (feat_img: the SR blocks' input, what their backward reads; res: the backward marches the forward's rays)
            # (batch: the frames; planes: the identities' — a multi-view backward expands them again for the renderer's adjoints —
            # ws_frames: the rows the SR blocks' styles were computed from)
            tape.update(backbone=bb_tape, sr=sr_tape, planes=planes_id, c=c, u_strat=u_strat, u_imp=u_imp,
                        feat_img=feat_sr, res=res, batch=b, planes_absmax=pam, ray_state=ray_state, views=views, ws_frames=ws)
            if geometry:      # the clamp range of the depth, for its adjoint (autograd.SynthesisFn.backward)
                tape["depth_range"] = ops.depth_range(tmm)
        return img, rgb_raw, depth.view(b, 1, res, res), wsum.view(b, 1, res, res) if geometry else None, normal, planes_id, feat_img

    def synthesis(self, ws: torch.Tensor, c: torch.Tensor, noise_mode: str = "const",
                  u_strat: Optional[torch.Tensor] = None, u_imp: Optional[torch.Tensor] = None,
                  return_planes: bool = False, geometry: bool = False, query: Optional[torch.Tensor] = None,
                  normals: bool = False, normal_grad: bool = False, normal_camera_grad: bool = False,
                  query_normals: bool = False, neural_rendering_resolution: Optional[int] = None,
                  **_unused) -> Dict[str, torch.Tensor]:
        """Drop-in for EG3D's TriPlaneGenerator.synthesis.  Differentiable w.r.t. `ws` (the latent-basis fitting of
        HFA-GP), w.r.t. the generator parameters that require grad (after `tune_generator()`) and w.r.t. the camera label `c`
        when it requires grad (pose refinement; the importance depths are detached as in EG3D).
        `geometry=True`: the dict also has 'image_mask' [B,1,r,r] (the per-ray opacity, sum of the compositing weights), and
        'image_depth' and 'image_mask' are differentiable — silhouette / matting losses and depth priors reach `ws` and the
        generator.  Off (the default), 'image_depth' carries no gradient and the dict has EG3D's three keys.
        `query=coords` [B or 1, M, 3] (world units): the dict also has 'query_sigma' [B,M,1] and 'query_rgb' [B,M,32], the raw
        decoder outputs at the points on THIS call's planes — the bits of `sample_mixed` under `no_grad` — differentiable w.r.t.
        `ws`, the generator parameters that require grad and `coords` when it requires grad.  Their gradient joins the
        renderer's before the one backbone backward pass: a point loss (EG3D's density regularisation, an occupancy prior) next
        to an image loss costs one launch, not a second backbone pass.  A loss on the points ALONE still runs the image's whole
        backward here (on a zero image gradient): `sample_mixed(..., differentiable=True)` is the cheaper form for that.
        `normals=True`: the dict also has 'image_normal' [B,3,r,r], the per-ray surface normal in WORLD space, pixel-aligned with
        'image_raw' / 'image_depth': N = Σ_s ω_s n_s with n = −∇σ·rsqrt(‖∇σ‖² + 1e-12) the unit normal of the raw density (from
        dense to empty) at every sample and ω the renderer's colour weights, so ‖N‖ ≤ 'image_mask'; not normalised
        (`render.normal_map` turns it into a picture).  With `normals=True` alone it is detached, inside a differentiable step
        too; the other outputs and their gradients are unchanged.
        `normal_grad=True` (implies `normals=True`): 'image_normal' is a differentiable output — normal-map supervision (a cosine
        or L1 term against an estimated or mesh normal map) reaches `ws` and the generator parameters that require grad, through
        the compositing weights and through the normals themselves (the second derivative of the tri-plane gather:
        ops.raymarch_normals_bwd, one launch that joins the renderer's plane and decoder gradients before the one backbone
        backward pass; a loss that does not touch 'image_normal' launches nothing extra).  It composes with `geometry=True` and
        `query=`.  The camera gradient of the normal term is opt-in: with `c.requires_grad` the call raises NotImplementedError
        unless `normal_camera_grad=True`.
        `normal_camera_grad=True` (implies `normal_grad=True`): a loss on 'image_normal' also reaches the camera label `c` when it
        requires grad — pose refinement with normal-map supervision.  ops.raymarch_normals_bwd_camera adds the normal term's per-ray
        records to those of ops.raymarch_bwd_camera and one reduction gives `c.grad` of the whole loss; a loss that does not touch
        'image_normal', or a `c` without grad, launches nothing extra.  The backward reads the ray marcher's saved per-sample state: a batch whose state exceeds
        RAY_STATE_CAP_BYTES raises RuntimeError (fitting batches are far below it).
        `query_normals=True` (with `query=`): the dict also has 'query_sigma_grad' [B,M,3], ∂σ/∂x of the raw density at the points in
        world units, and 'query_normal' [B,M,3], n = −∇σ·rsqrt(‖∇σ‖² + 1e-12) — the bits of `sample_mixed(normals=True)` — from the
        same single launch (ops.planes_query_normals), differentiable w.r.t. `ws` and the generator parameters that require grad:
        normal smoothness, gradient-norm penalties and normal agreement with a scan join the renderer's plane and decoder gradients
        (ops.planes_query_normals_bwd, after the query's own backward) before the one backbone backward pass; a loss that does not
        touch the two keys launches nothing extra.  It composes with `geometry=True` and `normals=True`.  The two outputs have no
        gradient w.r.t. the points: under grad a `query` that requires grad raises NotImplementedError, and so does the combination
        with `normal_grad=True` / `normal_camera_grad=True`.
        `neural_rendering_resolution=N` (EG3D's keyword): march N x N rays instead of the configured r0 x r0.  The value is stored in
        `self.neural_rendering_resolution`, as EG3D does, and holds for later calls; None (the default) reads that attribute.
        'image_raw', 'image_depth', 'image_mask', 'image_normal' and the 'feature_image' of `return_planes` are N x N; 'image' keeps
        its size: the feature image is resampled to r0 x r0 in front of the super-resolution blocks (ops.resize_aa: antialiased
        bilinear, as SuperresolutionHybrid8XDC does for rgb and x), and its adjoint (ops.resize_aa_bwd) hands the blocks' gradient
        back to the N x N rays, so every mode above composes.  N = 2 r0 supersamples (four rays per SR input pixel), N = r0 / 2 is
        EG3D's cheap training regime.  N outside [r0 / 4, 4 r0], or caller-given `u_strat` / `u_imp` that are not sized for N x N
        rays, raise ValueError before anything is launched; N = r0 launches exactly what a call without the keyword does.
        Multi-view: `c` [B,V,25] renders V cameras of every latent row on ONE backbone pass — a turntable, a stereo pair, the images
        of a capture rig at one time step, a multi-view consistency term.  The planes are computed once per identity; the ray
        marcher, the normals launch, the depth clamp, the resample and the SR blocks run at batch B·V (frame f = b·V + v, the SR
        blocks on the ws rows of identity b; memory grows with V as it does with B); the backward sums the views' plane gradients
        (ops.planes_sum_to_nhwc) and the SR blocks' style gradients and runs the backbone once at batch B, so every parameter
        reaches a trainer's gradient sink once.  The per-frame entries gain a view axis after the batch axis — 'image' [B,V,3,S,S],
        'image_raw' / 'image_normal' [B,V,3,r,r], 'image_depth' / 'image_mask' [B,V,1,r,r], 'feature_image' [B,V,r,r,32] — while
        'planes' stays [B,3,H,W,32] and the 'query_*' keys [B,M,·]: the points belong to the identity and are evaluated once.  `c.grad`
        is [B,V,25].  Caller-given uniforms are in frame order: `u_strat` B·V·r²·Sc elements, `u_imp` [B·V·r², Sf]; the depth clamp
        range is global over the B·V frames, as in `synthesis(ws.repeat_interleave(V, 0), c.flatten(0, 1))` — of which view v's
        'image_raw' / 'image_mask' / 'image_normal' are also the bits `synthesis(ws, c[:, v])` gives on that view's uniforms.  Every
        keyword above composes; RAY_STATE_CAP_BYTES counts B·V frames.  V = 0 gives empty tensors with the view axis, nothing
        launched; a label of any other rank, or one whose first axis is not B, raises ValueError.  A 2-D `c` is the call it always
        was: same launches, same bits."""
        return synthesis_call.synthesis(self, ws, c, noise_mode, u_strat, u_imp, return_planes, geometry, query, normals, normal_grad,
                                        normal_camera_grad, query_normals, neural_rendering_resolution)

    @torch.no_grad()
    def mapping(self, z: torch.Tensor, c: torch.Tensor, truncation_psi: float = 1.0) -> torch.Tensor:
        """EG3D MappingNetwork.forward (z, c) -> ws [B, num_ws, 512].  HFA-GP never calls it (its ws come from the
        latent basis, headnerf.py:81-102); provided for unconditional sampling.  Inference only."""
        cfg = self.cfg
        mp = self.backbone.mapping

        def norm2(x):       # normalize_2nd_moment: tiny host-side glue
            return x * (x.square().mean(1, keepdim=True) + 1e-8).rsqrt()
        x = norm2(z.float().contiguous())
        y = norm2(ops.fully_connected(c.float().contiguous(), mp.embed.weight, mp.embed.bias))
        x = torch.cat([x, y], 1).contiguous()
        for i in range(cfg.mapping_layers):
            fc = getattr(mp, f"fc{i}")
            x = ops.fully_connected(x, fc.weight, fc.bias, cfg.mapping_lr_mul, act="lrelu", alpha=0.2)
        ws = x[:, None].repeat(1, cfg.num_ws, 1)
        if truncation_psi != 1.0:
            ws = mp.w_avg.lerp(ws, truncation_psi)
        return ws

    # ------------------------------------------------------------------ point queries (EG3D TriPlaneGenerator.sample*)
    def _query_guard(self, who: str, ws: torch.Tensor, *tensors, differentiable: bool = False) -> None:
        if not ws.is_cuda:
            raise RuntimeError(f"TriPlaneGenerator.{who}: the MI355X path needs CUDA/ROCm tensors; there is no CPU fallback")
        if ws.device.index != torch.cuda.current_device():
            raise RuntimeError(f"TriPlaneGenerator.{who}: tensors live on {ws.device} but the current device is "
                               f"cuda:{torch.cuda.current_device()}; wrap the call in `with torch.cuda.device(ws.device):`")
        if ws.dim() != 3 or ws.shape[1:] != (self.cfg.num_ws, self.cfg.w_dim):
            raise ValueError(f"expected ws [B,{self.cfg.num_ws},{self.cfg.w_dim}], got {tuple(ws.shape)}")
        if not differentiable:
            self._no_backward(who, ws, *tensors)

    def _no_backward(self, who: str, *tensors) -> None:
        if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors) or
                                        any(p.requires_grad for p in self.parameters())):
            hint = " — or pass `differentiable=True`, or ride on an image pass with `synthesis(query=)`" if who == "sample_mixed" \
                else ""
            raise RuntimeError(f"TriPlaneGenerator.{who}: wrap in `torch.no_grad()`; the query has no backward "
                               f"(an input or a generator parameter requires grad){hint}")

    def _query_planes(self, ws: torch.Tensor):
        """One backbone pass → (planes [B,3,R,R,32], the |planes| bound `synthesis` hands the renderer)."""
        planes = self.backbone_planes(ws.detach().float().contiguous())
        return planes, getattr(self, "_planes_absmax", None)

    def _query_kwargs(self) -> dict:
        cfg = self.cfg
        return dict(zip(ops._DEC, self.decoder_params()), box_warp=cfg.box_warp, plane_axes=ops._plane_axes_id(cfg.plane_axes),
                    decoder_lr_mul=cfg.decoder_lr_mul, decoder_precision=cfg.decoder_precision)

    def sample_mixed(self, coordinates: torch.Tensor, directions: Optional[torch.Tensor], ws: torch.Tensor,
                     truncation_psi=1, truncation_cutoff=None, update_emas=False, *, differentiable: bool = False,
                     normals: bool = False, **synthesis_kwargs) -> Dict[str, torch.Tensor]:
        """EG3D TriPlaneGenerator.sample_mixed: the raw decoder outputs at `coordinates` [B or 1, M, 3] (world units) of the
        tri-planes of `ws` → {'rgb': [B,M,32], 'sigma': [B,M,1]} (sigma before the renderer's softplus).  `directions` is
        shape-checked and ignored (OSGDecoder does not read it); the truncation arguments are EG3D's and unused here, as
        there.  One backbone pass, one launch (ops.planes_query), the decoder precision the renderer runs.
        Forward only unless `differentiable=True`: then, under grad, the outputs are differentiable w.r.t. `ws`, the generator
        parameters that require grad and `coordinates` when it requires grad, at the price of a backbone backward pass of its
        own — a loss that also renders should use `synthesis(query=)`, which shares the image's pass.  Inside a trainer step
        scope (a gradient sink, or gradients accumulated in place) the stand-alone form raises: a second pass would hand every
        parameter to the sink twice.
        `normals=True`: the dict also has 'sigma_grad' [B,M,3], ∂σ/∂x of the raw density in world units, and 'normal' [B,M,3],
        n = −∇σ·rsqrt(‖∇σ‖² + 1e-12) (from dense to empty; exact zeros outside every plane), from the same single launch
        (ops.planes_query_normals; 'sigma' / 'rgb' keep their bits).  With `differentiable=True` both are differentiable w.r.t. `ws`
        and the generator parameters that require grad (ops.planes_query_normals_bwd), NOT w.r.t. the points: under grad,
        `coordinates` that require grad raise NotImplementedError."""
        noise_mode = synthesis_kwargs.get("noise_mode", "const")
        if noise_mode != "const":
            raise NotImplementedError("HFA-GP always passes noise_mode='const' (headnerf.py:112)")
        if coordinates.dim() != 3 or coordinates.shape[-1] != 3 or coordinates.shape[0] not in (1, ws.shape[0]):
            raise ValueError(f"expected coordinates [B or 1, M, 3] for ws of batch {ws.shape[0]}, got {tuple(coordinates.shape)}")
        if directions is not None and directions.shape != coordinates.shape:
            raise ValueError(f"directions {tuple(directions.shape)} must match coordinates {tuple(coordinates.shape)}")
        params = [p for n, p in self.named_parameters() if not n.startswith("backbone.mapping.")]
        grad = differentiable and torch.is_grad_enabled() and (ws.requires_grad or coordinates.requires_grad or
                                                               any(p.requires_grad for p in params))
        if normals:
            if torch.is_grad_enabled() and coordinates.requires_grad:
                raise NotImplementedError("TriPlaneGenerator.sample_mixed(normals=True): 'sigma_grad' / 'normal' have no gradient w.r.t. "
                                          "the points (it needs the mixed second derivative of the gather); detach `coordinates`")
            if not coordinates.is_cuda:
                raise RuntimeError("TriPlaneGenerator.sample_mixed: the MI355X path needs CUDA/ROCm tensors; there is no CPU fallback")
        self._query_guard("sample_mixed", ws, *(() if differentiable else (coordinates,)), differentiable=differentiable)
        b, m = ws.shape[0], coordinates.shape[1]
        if b == 0 or m == 0:
            zero = 0.0 * ws.sum() + 0.0 * coordinates.sum() if grad else 0.0       # keeps the autograd edges
            out = {"rgb": torch.zeros(b, m, 32, device=ws.device) + zero, "sigma": torch.zeros(b, m, 1, device=ws.device) + zero}
            if normals:
                out.update(sigma_grad=torch.zeros(b, m, 3, device=ws.device) + zero, normal=torch.zeros(b, m, 3, device=ws.device) + zero)
            return out
        if grad:
            if getattr(self, "_grad_sink", None) is not None or getattr(self, "_grad_inplace", False):
                raise RuntimeError("TriPlaneGenerator.sample_mixed(differentiable=True) inside a trainer step scope: its backward is "
                                   "a second backbone pass and would release every parameter to the gradient sink twice — "
                                   "evaluate the points with `synthesis(..., query=coordinates)` instead")
            if not coordinates.is_cuda:
                raise RuntimeError("TriPlaneGenerator.sample_mixed: the MI355X path needs CUDA/ROCm tensors; there is no CPU fallback")
            from .autograd import SampleMixedFn
            sigma, rgb, sigma_grad, normal = SampleMixedFn.apply(ws, coordinates, bool(normals), self, *params)
            out = {"rgb": rgb, "sigma": sigma}
            if normals:
                out.update(sigma_grad=sigma_grad, normal=normal)
            return out
        with torch.no_grad():
            planes, pam = self._query_planes(ws)
            if normals:
                q = self._timed("planes_query_normals", float(b), ops.planes_query_normals, planes,
                                coordinates.detach().float().contiguous(), planes_absmax=pam, **self._query_kwargs())
                return {"rgb": q["rgb"], "sigma": q["sigma"], "sigma_grad": q["grad"], "normal": q["normal"]}
            sigma, rgb = ops.planes_query(planes, coordinates.detach().float().contiguous(), planes_absmax=pam,
                                          **self._query_kwargs())
        return {"rgb": rgb, "sigma": sigma}

    # ------------------------------------------------------------------ explicit ray lists (EG3D ImportanceRenderer.forward's rays)
    def _rays_kwargs(self) -> dict:
        """`_render_args` without the camera: what ops.raymarch_rays* take next to the planes, the rays and the uniforms."""
        cfg = self.cfg
        return dict(zip(ops._DEC, self.decoder_params()), ray_start=cfg.ray_start, ray_end=cfg.ray_end, box_warp=cfg.box_warp,
                    decoder_lr_mul=cfg.decoder_lr_mul, plane_axes=ops._plane_axes_id(cfg.plane_axes), white_back=cfg.white_back,
                    decoder_precision=cfg.decoder_precision)

    def render_rays(self, ws: torch.Tensor, ray_origins: torch.Tensor, ray_directions: torch.Tensor,
                    u_strat: Optional[torch.Tensor] = None, u_imp: Optional[torch.Tensor] = None,
                    noise_mode: str = "const", t_near=None, t_far=None, ray_limits=None, normals: bool = False,
                    normal_grad: bool = False, normal_ray_grad: bool = False, samples: bool = False,
                    compact: bool = False) -> Dict[str, torch.Tensor]:
        """The renderer of `synthesis` on caller-given rays: ray_origins / ray_directions [B,R,3] in world units, R arbitrary — a
        crop or zoomed window (`cam_utils.ray_grid(c, res, window=)`), several cameras of one identity as one longer list in that
        frame (`torch.cat` along dim 1), random ray batches, or any camera model written in torch.  Directions are taken as given,
        not normalised: a sample is o + t·d with t in the config's [ray_start, ray_end], as EG3D's renderer takes them.
        → {'feature' [B,R,32], 'rgb' [B,R,3] (the first three features), 'depth' [B,R] (clamped to this call's global sample range,
        as 'image_depth' is), 'mask' [B,R] (opacity)}.  One backbone pass, one launch (ops.raymarch_rays); no super-resolution.
        Under grad the four are differentiable w.r.t. `ws`, the generator parameters that require grad and the rays (so a label
        `c` gets its gradient through `ray_grid` from torch autograd), at the price of a backbone backward pass of its own; inside a
        trainer step scope it raises, as `sample_mixed(differentiable=True)` does.  `u_strat` [B,R,Sc] / `u_imp` [B·R,Sf]: the
        uniforms of the two sampling passes (drawn here when None).  R = 0 or B = 0: empty tensors, nothing is launched.
        Per-ray depth limits — a camera at any distance, directions of any length, visibility rays, depth-guided sampling:
        `t_near` / `t_far` (tensors [B,R] or Python floats, both or neither) sample ray i on [t_near_i, t_far_i] instead of the
        config's interval; `ray_limits="box"` takes them from the rays' intersection with the tri-plane cube of side cfg.box_warp
        (`ops.ray_limits_box`; EG3D's ray_start = ray_end = 'auto', but t_near is clamped at 0: an origin inside the cube starts
        at the origin).  The dict then also has 'valid' [B,R] bool: both limits finite and t_far > t_near.  Any other ray is EMPTY
        and is not marched: 'feature' is the background (−1, or +1 with white_back), 'mask' 0 and 'depth' the upper end of the
        call's clamp range — what EG3D's zero-opacity ray gets (0 if no ray is valid); nothing in the dict is NaN or inf.  The limits
        are NOT differentiated (a limit that requires grad raises; "box" computes them from detached rays): the rays' gradient is
        the derivative with the limits held fixed — EG3D's autograd also moves the sample positions through the box intersection;
        leaving that term out is deliberate, as for the importance depths — and an empty ray gets exactly zero gradient.
        Surface normals, with the keywords of `synthesis`: `normals=True` adds 'normal' [B,R,3], per ray N = Σ_s ω_s n_s — world
        space, not normalised, ‖N‖ ≤ 'mask', `white_back` does not enter ('image_normal' of `synthesis`, per ray); exactly 0 for an
        empty ray.  One more launch (ops.raymarch_rays_normals) on the per-sample state of the march, which a call whose state
        exceeds RAY_STATE_CAP_BYTES runs in chunks of rays under no_grad.  It is detached unless `normal_grad=True` (which implies
        `normals`): 'normal' is then differentiable w.r.t. `ws` and the generator parameters that require grad, the four decoder
        tensors included, at one more backward launch, and only when the loss uses it; above the cap that raises RuntimeError.  The
        rays get the normal term's gradient only with `normal_ray_grad=True` (which implies `normal_grad`) — rays that require
        grad raise NotImplementedError without it, as a label does in `synthesis(normal_grad=True)` without
        `normal_camera_grad=True`.  The sample depths and the limits carry no gradient here either.
        The distribution along the ray: `samples=True` adds 'sample_depths' [B,R,S] — the S = Sc + Sf sample depths of the ray, sorted
        ascending — and 'sample_weights' [B,R,S−1], the compositing weight w_e = α_e·T_e of the interval [t_e, t_{e+1}]: the values
        the kernel composites with, so Σ_e w_e is 'mask' and Σ_e w_e (t_e + t_{e+1})/2 / Σ_e w_e the depth before its clamp;
        `white_back` does not enter.  For a distortion loss, a depth-distribution loss against a scan, median / quantile depth, depth
        variance, transmittance at a depth (`ray_losses`).  Same launch count (ops.raymarch_rays(samples=True)); the four other
        entries keep their bits.  'sample_depths' is always DETACHED — EG3D detaches the importance depths and the stratified ones
        are constants of the uniforms — and so are the limits; under grad 'sample_weights' is differentiable w.r.t. `ws`, the
        generator parameters that require grad (decoder included) and the rays (limits held fixed), its gradient entering the one
        ray-march backward launch of the colour term, which then runs even when only 'sample_weights' carries a gradient.  An empty
        ray has zeros in both (not inf: w·t stays finite in a loss).  It composes with the limits, with the three normal keywords
        and with a state above RAY_STATE_CAP_BYTES; R = 0 gives [B,0,S] / [B,0,S−1].  `synthesis` has no such keyword: its grid as a
        list (`cam_utils.ray_grid`) renders what it renders.
        Empty space: `ray_limits=occ` with an `OccupancyGrid` (`occupancy_grid`, or `OccupancyGrid.from_dense` of any mask; batch B
        or 1, cube_length == cfg.box_warp) takes the limits from the grid instead of the cube — per ray the entry of the first and
        the exit of the last occupied cell (`ops.ray_limits_grid`, under no_grad from detached rays, as "box"), so the samples
        are spent on the head's chord and a ray that meets no occupied cell is empty.  The same launches as `t_near=` / `t_far=`
        run, and every keyword composes.  ONE interval per ray: empty cells between occupied ones are still sampled.
        `compact=True` (only with limits of any kind): per frame the valid rays are moved to the front (stable: their order is
        kept), only the first R' = the largest valid count of a frame are marched (plus one empty ray, which costs nothing and
        carries the depth an empty ray gets), and the results are scattered back — the forward entries are bit-identical to
        `compact=False`, since a ray's result depends on its own inputs only; the rays' gradient comes through the gather from torch
        autograd.  It costs one host sync (R' is a Python int); no valid ray at all launches nothing."""
        from . import ray_list
        return ray_list.render_rays(self, ws, ray_origins, ray_directions, u_strat, u_imp, noise_mode, t_near, t_far, ray_limits,
                                    normals, normal_grad, normal_ray_grad, samples, compact)

    def trace_rays(self, ws: torch.Tensor, ray_origins: torch.Tensor, ray_directions: torch.Tensor, level: float = 10.0,
                   steps: int = 128, refine: int = 8, t_near=None, t_far=None, ray_limits=None, normals: bool = True,
                   differentiable: bool = False) -> Dict[str, torch.Tensor]:
        """Where each ray of a list first meets the density iso-surface σ = `level` — the surface `extract_mesh(level=)` exports, in
        the unit of `sample_mixed`'s 'sigma' (before any softplus): a 2-D landmark to a 3-D point on the head
        (`cam_utils.pixel_rays`), a depth map that agrees with the mesh, shadow-ray origins, depth against a range scan.  Rays
        [B,R,3] as `render_rays` takes them (directions not normalised: a point is o + t·d).  →
          'hit' [B,R] bool, 'cell' [B,R] int32: the first node i of t_i = t_near + i·(t_far − t_near)/steps, i = 0 … steps, with
                σ ≥ level; −1 for a miss, 0 when the ray starts inside (then t = t_near);
          't' [B,R]: for cell > 0 the root inside [t_{cell−1}, t_cell] after `refine` bisections and one secant step — within
                (t_far − t_near)/(steps·2^refine) of the crossing the coarse march bracketed; a surface thinner than one step
                between two nodes is stepped over;
          'point' [B,R,3] = o + t·d, 'sigma' [B,R] the density there, and with `normals` 'sigma_grad' [B,R,3] = ∂σ/∂x and 'normal'
                [B,R,3] = −∇σ·rsqrt(‖∇σ‖² + 1e-12): the bits of `sample_mixed(point, normals=True)`.
        A miss has exact zeros in every float entry.  One backbone pass, one launch (ops.trace_rays), no atomics: two calls give the
        same bits.  R = 0 or B = 0: empty tensors, nothing is launched.
        The limits resolve exactly as in `render_rays`: the config's [ray_start, ray_end], `t_near` / `t_far` (tensors [B,R] or
        floats), `ray_limits="box"` or an `OccupancyGrid`; with any of them the dict has 'valid' [B,R], and a ray that is not valid
        is a miss.  As there, the limits are NOT differentiated, and neither is `level`.
        `differentiable=True`: under grad 't' and 'point' are differentiable w.r.t. `ws`, the generator parameters that require grad
        and the rays, by the implicit function theorem — dt = −dσ(x*)/(g·d) at the traced root, evaluated through the differentiable
        point query (`ray_losses.implicit_depth` on `sample_mixed(differentiable=True)`; no further kernel).  A ray carries this
        gradient only if it is a hit with cell > 0 whose crossing is transversal, g·d ≥ 0.01·‖g‖‖d‖; every other ray — a miss, a start
        inside, a grazing crossing — has constant 't' and 'point': exactly zero gradient.  The other entries are detached.  The call
        pays a backbone backward pass of its own; inside a trainer step scope it raises, as `sample_mixed(differentiable=True)` does:
        there, trace under no_grad and pass 'point' through `synthesis(query=)` with `ray_losses.implicit_depth`."""
        from . import ray_list
        return ray_list.trace_rays(self, ws, ray_origins, ray_directions, level, steps, refine, t_near, t_far, ray_limits, normals,
                                   differentiable)

    def sample(self, coordinates: torch.Tensor, directions: Optional[torch.Tensor], z: torch.Tensor, c: torch.Tensor,
               truncation_psi=1, truncation_cutoff=None, update_emas=False, **synthesis_kwargs) -> Dict[str, torch.Tensor]:
        """EG3D TriPlaneGenerator.sample: `mapping(z, c, truncation_psi)` then `sample_mixed`.  Only truncation_cutoff=None
        (truncate every w row) is supported."""
        if truncation_cutoff is not None:
            raise NotImplementedError("TriPlaneGenerator.sample: only truncation_cutoff=None is supported")
        self._no_backward("sample", z, coordinates)
        ws = self.mapping(z, c, truncation_psi=truncation_psi)
        return self.sample_mixed(coordinates, directions, ws, update_emas=update_emas, **synthesis_kwargs)

    def density_grid(self, ws: torch.Tensor, resolution: int = 512, cube_length: Optional[float] = None,
                     max_points: Optional[int] = None) -> torch.Tensor:
        """Raw density on EG3D's shape-export lattice (gen_samples.py --shapes, create_samples): [B, N, N, N] indexed (ix, iy, iz),
        iz fastest, N = `resolution` points per axis over a cube of side `cube_length` (default box_warp) centred at the
        origin — before EG3D's flip / border trim (render.shape_volume_eg3d).  The lattice is the exact integer one
        (DESIGN.md §4.4).  One backbone pass, then the grid-mode kernel in x slabs of at most `max_points` points (at
        least one x plane per launch); no coordinate tensor is built.  Forward only."""
        n = int(resolution)
        if n < 2:
            raise ValueError(f"density_grid: resolution must be >= 2, got {resolution}")
        self._query_guard("density_grid", ws)
        b = ws.shape[0]
        vol = torch.empty(b, n, n, n, device=ws.device, dtype=torch.float32)
        if b == 0:
            return vol
        cube = float(self.cfg.box_warp if cube_length is None else cube_length)
        with torch.no_grad():
            planes, pam = self._query_planes(ws)
            self._fill_density(vol, planes, pam, cube, max_points)
        return vol

    def occupancy_grid(self, ws: torch.Tensor, resolution: int = 64, level: float = 0.0, oversample: int = 2, dilate: int = 1,
                       cube_length: Optional[float] = None, max_points: Optional[int] = None):
        """An `OccupancyGrid` of the heads of `ws` for `render_rays(..., ray_limits=occ)`: G = `resolution` (2 … 256) cells per axis
        over a cube of side `cube_length` (default box_warp — the only one `render_rays` takes).  One backbone pass; the raw density
        on the exact integer lattice of n = G·k + 1 points per axis, k = `oversample` ≥ 1 (`density_grid`'s kernel), then ONE launch
        (ops.occupancy_pack): a cell is occupied iff one of the (k+1)³ lattice points of its closed extent has !(σ < level) — faces
        are shared with the neighbours, which errs on the conservative side; a NaN is occupied — and the grid is dilated by
        `dilate` cells (0 … 8).  Forward only.
        `level` is the caller's trade-off between tight limits and lost density: it is compared with the RAW σ of `sample_mixed`,
        which enters the march as softplus(σ − 1) — at σ = 0 that is still 0.31 per unit length.  With trained EG3D weights empty
        space is strongly negative and a level around 0 keeps every visible sample; with random weights no level is meaningful.
        The field is only seen at the lattice points: `oversample` and `dilate` are the margin for what lies between them."""
        from .occupancy import OccupancyGrid
        g, k = int(resolution), int(oversample)
        if not 2 <= g <= 256:
            raise ValueError(f"occupancy_grid: resolution must be in [2, 256], got {resolution}")
        if k < 1 or g * k + 1 > 1025:
            raise ValueError(f"occupancy_grid: oversample must be >= 1 with resolution * oversample + 1 <= 1025, got {oversample}")
        if not 0 <= int(dilate) <= 8:
            raise ValueError(f"occupancy_grid: dilate must be in [0, 8], got {dilate}")
        self._query_guard("occupancy_grid", ws)
        b, n = ws.shape[0], g * k + 1
        cube = float(self.cfg.box_warp if cube_length is None else cube_length)
        if b == 0:
            return OccupancyGrid(torch.zeros(0, g, g, (g + 31) // 32, device=ws.device, dtype=torch.int32), g, cube)
        with torch.no_grad():
            vol = torch.empty(b, n, n, n, device=ws.device, dtype=torch.float32)
            planes, pam = self._query_planes(ws)
            self._fill_density(vol, planes, pam, cube, max_points)
            bits = self._timed("occupancy_pack", float(b), ops.occupancy_pack, vol, g, k, float(level), int(dilate))
        return OccupancyGrid(bits, g, cube)

    def _fill_density(self, vol: torch.Tensor, planes: torch.Tensor, pam, cube: float, max_points: Optional[int]) -> None:
        b, n = vol.shape[0], vol.shape[1]
        step = n if max_points is None else max(1, min(n, int(max_points) // (b * n * n)))
        kw = self._query_kwargs()
        for x0 in range(0, n, step):
            xc = min(step, n - x0)
            ops.planes_query(planes, grid=(n, cube, x0, xc), planes_absmax=pam, want_rgb=False,
                             out=vol[:, x0:x0 + xc], **kw)

    def extract_mesh(self, ws: torch.Tensor, resolution: int = 512, level: float = 10.0, cube_length: Optional[float] = None,
                     max_points: Optional[int] = None, colors: bool = False, normals: bool = False):
        """Surface meshes of the heads of `ws`: `density_grid`, EG3D's border trim (voxels within int(30 N / 256) of a face
        set to -1000; no flip), then marching cubes at `level` (ops.marching_cubes) with the lattice spacing
        cube_length / (N - 1) and origin -cube_length / 2, so vertices are in WORLD units (the frame `sample_mixed` takes).
        Returns one dict per identity: {'vertices' [V, 3] float32, 'faces' [F, 3] int32}, plus 'colors' [V, 3] uint8 when
        `colors`: the first three decoder features at the vertices (ops.planes_query, as `sample_mixed`), quantised as
        render.to_uint8 quantises image_raw; plus 'normals' [V, 3] float32 when `normals`: the analytic unit normal
        −∇σ·rsqrt(‖∇σ‖² + 1e-12) of the density field at the vertices (one ops.planes_query_normals call on the planes already
        computed), pointing from dense to empty — the side marching cubes winds its faces toward.  One backbone pass.  Forward only."""
        from .render import _border_eg3d, to_uint8
        n = int(resolution)
        if n < 2:
            raise ValueError(f"extract_mesh: resolution must be >= 2, got {resolution}")
        self._query_guard("extract_mesh", ws)
        b = ws.shape[0]
        cube = float(self.cfg.box_warp if cube_length is None else cube_length)
        voxel = cube / (n - 1)
        out = []
        if b == 0:
            return out
        with torch.no_grad():
            planes, pam = self._query_planes(ws)
            vol = torch.empty(b, n, n, n, device=ws.device, dtype=torch.float32)
            self._fill_density(vol, planes, pam, cube, max_points)
            for i in range(b):
                verts, faces = ops.marching_cubes(_border_eg3d(vol[i]), level, spacing=(voxel,) * 3, origin=(-cube / 2,) * 3)
                mesh = {"vertices": verts, "faces": faces}
                if colors:
                    rgb = torch.zeros(verts.shape[0], 32, device=ws.device)
                    if verts.shape[0]:
                        rgb = ops.planes_query(planes[i:i + 1], verts[None], planes_absmax=pam, **self._query_kwargs())[1][0]
                    mesh["colors"] = to_uint8(rgb[:, :3])
                if normals:
                    mesh["normals"] = ops.planes_query_normals(planes[i:i + 1], verts[None], want=("normal",), planes_absmax=pam,
                                                               **self._query_kwargs())["normal"][0]
                out.append(mesh)
        return out

    def forward(self, *args, **kwargs):
        raise NotImplementedError("HFA-GP only calls generator.synthesis (headnerf.py:112); mapping is in mapping()")


def load_G_official(args=None, device="cuda", cfg: Optional[GeneratorConfig] = None, seed: int = 0,
                    weights: Optional[str] = None) -> TriPlaneGenerator:
    """Counterpart of headnerf.py:31-38.  The EG3D pickle is not shipped with the reference, so the
    generator is random-initialised from ``seed`` (EG3D init) or loaded from a safetensors file with
    EG3D key names; it comes back frozen, as the reference does (``requires_grad_(False)``)."""
    if cfg is None and getattr(args, "generator_preset", None):
        from .config import PRESETS
        cfg = PRESETS[args.generator_preset]()
    seed = getattr(args, "generator_seed", seed)
    weights = weights or getattr(args, "generator_weights", None)
    g = TriPlaneGenerator(cfg, seed=seed)
    if weights is not None:
        from safetensors.torch import load_file
        g.load_state_dict(load_file(weights), strict=True)
    return g.requires_grad_(False).to(device)

"""Operator layer: the EG3D op API of the hot path, backed by libhfagp_hip.so.

Mirrors (names and argument meaning) the operators the reference's generator
reaches below ``generator.synthesis`` (headnerf.py:112): ``bias_act``,
``upfirdn2d`` / ``upsample2d``, ``modulated_conv2d`` (+ fused ``bias_act``),
and the renderer.  Every function takes CUDA (ROCm) fp32 tensors, enqueues on
``torch.cuda.current_stream()`` and never falls back to PyTorch math.
Activations are channels-last ``[B, H, W, C]`` unless a name says ``nchw``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import types
from typing import Optional, Tuple

import torch

from . import _lib as L

CONV3X3, CONVT3X3_UP2, CONV1X1, CONV3X3_BWD, CONVS2_BWD = 0, 1, 2, 3, 4
ACT_LINEAR, ACT_LRELU = 0, 1
_ACT = {"linear": ACT_LINEAR, "lrelu": ACT_LRELU}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """hipStream_t of torch's current stream on the current device.  The raw accessor is ~20x cheaper than
    ``torch.cuda.current_stream()`` (which builds a Stream object): it is called once per launch, ~350 times per
    fitting step."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t


def _chk_act(t: torch.Tensor, name: str) -> torch.Tensor:
    """An activation: float32 (`_chk`), or float16 storage — a contiguous device tensor read / written as stored."""
    if t.dtype != torch.float16:
        return _chk(t, name)
    if not (t.is_cuda and t.is_contiguous()):
        raise RuntimeError(f"{name}: expected a contiguous CUDA/ROCm tensor")
    return t


def _clamp(clamp: Optional[float]) -> float:
    """The library's clamp encoding: a negative value = no clamp."""
    return -1.0 if clamp is None else float(clamp)


# The library sees pointers and integers, never a tensor's extent: for the streaming ops below these two checks are the only guard
# between a mis-shaped operand and a kernel that reads or writes past it.  Shape tuples and dtypes only: they sit on the per-layer path.
def _chk_operand(who: str, name: str, t: Optional[torch.Tensor], shape, like: torch.Tensor) -> Optional[torch.Tensor]:
    """An optional fp32 operand of exactly `shape`, contiguous, on the device of `like`."""
    if t is None:
        return None
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != like.device or not t.is_contiguous():
        raise RuntimeError(f"{who}: {name} must be a contiguous float32 tensor {list(shape)} on {like.device}, got "
                           f"{list(t.shape)} {t.dtype} on {t.device}")
    return t


def _chk_absmax(who: str, name: str, t: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    """An optional slot buffer of the fp16 range tracking (`absmax_slots`): at least HFAGP_ABSMAX_FLOATS floats."""
    if t is None:
        return None
    if t.numel() < L.ABSMAX_FLOATS or t.dtype != torch.float32 or t.device != like.device or not t.is_contiguous():
        raise RuntimeError(f"{who}: {name} must be a contiguous float32 buffer of at least {L.ABSMAX_FLOATS} floats on {like.device}, "
                           f"got {list(t.shape)} {t.dtype} on {t.device}")
    return t


# ----------------------------------------------------------------------------- weights
def weight_prep(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """weight [Cout, Cin, k, k] → (wt [k*k, Cin/4, Cout, 4], wsq [Cout, Cin])."""
    _chk(weight, "weight")
    co, ci, kh, kw = weight.shape
    wt = torch.empty(kh * kw, ci // 4, co, 4, device=weight.device, dtype=torch.float32)
    wsq = torch.empty(co, ci, device=weight.device, dtype=torch.float32)
    L.check(L.lib().hfagp_weight_prep(_ptr(weight), _ptr(wt), _ptr(wsq), co, ci, kh * kw, _stream()), "weight_prep")
    return wt, wsq


PREC_F32, PREC_BF16X3, PREC_BF16X6, PREC_F16, PREC_F16X3, PREC_F16X2 = 0, 1, 2, 3, 4, 5
# "f16x2" (TF32 class, NOT the default): the f16x3 weight image against activations rounded to one fp16 part — 2 MFMAs / product
PRECISIONS = {"fp32": PREC_F32, "bf16x3": PREC_BF16X3, "bf16x6": PREC_BF16X6, "f16": PREC_F16, "f16x3": PREC_F16X3,
              "f16x2": PREC_F16X2}
NPARTS = {"fp32": 0, "f16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 2, "f16x2": 2}   # parts of the 16-bit weight image (0: fp32 image)
_IMAGE_DTYPE = {"f16": torch.float16, "f16x3": torch.float16, "f16x2": torch.float16, "bf16x3": torch.bfloat16,
                "bf16x6": torch.bfloat16}


def split_supported(cin: int, cout: int, up: bool = False) -> bool:
    """Shapes the 16-bit conv paths take (hfagp.h: Cin % 16 == 0 and Cout % 128 == 0, or Cout % 128 >= 96 for the
    non-upsampling modes: the 96-channel toRGB on a 128-wide tile whose last 32 columns are discarded)."""
    return cin % 16 == 0 and (cout % 128 == 0 or (cout % 128 >= 96 and not up))


def weight_prep_prec(weight: torch.Tensor, precision: str) -> torch.Tensor:
    """weight [Cout, Cin, k, k] fp32 → B-operand image [parts, k*k, Cin/8, Cout, 8] of a 16-bit conv precision:
    'bf16x3' / 'bf16x6' = 2 / 3 bfloat16 parts, 'f16x3' = 2 float16 parts (each part the round-to-nearest value of
    the residual left by the parts before it), 'f16' = one float16 part.
    The float16 kinds are SCALED images (include/hfagp.h "Weight images"): the parts of w * 2^-e, e the multiple of 8 that brings
    max |w| of the tensor into [2^-4, 2^4) (0 for unit-scale weights), so their accuracy class does not depend on the weight's scale.  max |w| stays on the device, in
    ``image.w_absmax`` (one float): `modconv` / `upconv_fir` / `torgb_skip` pass it on with the image, so hand them the returned
    tensor itself — a copy or a view of it would be taken for an image of the raw weight (`weight_prep_split` makes those)."""
    return _weight_prep_prec(weight, precision, scaled=_IMAGE_DTYPE[precision] == torch.float16)


def _weight_prep_prec(weight: torch.Tensor, precision: str, scaled: bool) -> torch.Tensor:
    _chk(weight, "weight")
    co, ci, kh, kw = weight.shape
    nparts = NPARTS[precision]
    # + 512 B behind the image: with Cout % 128 != 0 the 128-wide tile reads one partial row past it (hfagp.h).  Only readable
    # memory is needed there — the columns fed from it are never stored — so nothing is cleared (the RGB fitting step re-builds
    # 21 images per step: clearing them was 0.24 ms of fill kernels).  INVARIANT the kernels keep: no consumer reduces over the
    # discarded columns (each output column of the GEMM depends on its own B column only; the fused toRGB sums and the absmax
    # reduction run over stored columns) — tests/test_gpu_parity.py::test_torgb96_on_padded_split_tile runs with the pad poisoned.
    numel = nparts * kh * kw * (ci // 8) * co * 8
    flat = torch.empty(numel + 256, device=weight.device, dtype=_IMAGE_DTYPE[precision])
    wb = flat[:numel].view(nparts, kh * kw, ci // 8, co, 8)
    if scaled:
        wb.w_absmax = torch.empty(1, device=weight.device, dtype=torch.float32)
        L.check(L.lib().hfagp_weight_prep_scaled(_ptr(weight), wb.data_ptr(), _ptr(wb.w_absmax), co, ci, kh * kw,
                                                 PRECISIONS[precision], _stream()), "weight_prep_scaled")
    else:
        L.check(L.lib().hfagp_weight_prep_prec(_ptr(weight), wb.data_ptr(), co, ci, kh * kw, PRECISIONS[precision], _stream()),
                "weight_prep_prec")
    return wb


def weight_prep_batch_supported(weight: torch.Tensor) -> bool:
    co, ci, kh, kw = weight.shape
    return co % 32 == 0 and ci % 32 == 0 and kh == kw and kh in (1, 3)


def weight_prep_batch(items):
    """items: [(weight [Cout,Cin,k,k], precision | None, precision_t | None, want_wsq)] -> [(image | None, image_t | None, wsq | None)]
    in ONE launch per 48 weights (hfagp_weight_prep_batch): the forward image, the image of the Cin/Cout transpose and wsq of every
    weight from a single read of it.  All outputs of a call live in three flat buffers (one allocation each), max |w| of the items
    with a float16 image (scaled images, `weight_prep_prec`: ``image.w_absmax``) in a fourth."""
    metas, n16 = [], {torch.float16: 0, torch.bfloat16: 0}
    nsq = 0
    for w, prec, prec_t, want_wsq in items:
        _chk(w, "weight")
        co, ci, kh, kw = w.shape
        sizes = []
        for pr in (prec, prec_t):
            if pr is None:
                sizes.append(None)
            else:
                dt = _IMAGE_DTYPE[pr]
                numel = NPARTS[pr] * kh * kw * ci * co            # (same element count for the transpose)
                sizes.append((dt, n16[dt], numel))
                n16[dt] += (numel + 256 + 7) // 8 * 8            # + the 512-byte readable pad behind an image (see weight_prep_prec)
        metas.append((sizes, nsq if want_wsq else None))
        if want_wsq:
            nsq += co * ci
    dev = items[0][0].device
    flat = {dt: torch.empty(n, device=dev, dtype=dt) for dt, n in n16.items() if n}
    sq = torch.empty(nsq, device=dev, dtype=torch.float32) if nsq else None
    amax = torch.empty(len(items), device=dev, dtype=torch.float32) if torch.float16 in flat else None
    out, arr = [], (L.WeightPrepItem * len(items))()
    for k, ((w, prec, prec_t, want_wsq), (sizes, sq_off)) in enumerate(zip(items, metas)):
        co, ci, kh, kw = w.shape
        views = []
        for pr, sz, shape in ((prec, sizes[0], (kh * kw, ci // 8, co, 8)), (prec_t, sizes[1], (kh * kw, co // 8, ci, 8))):
            if sz is None:
                views.append(None)
            else:
                dt, off, numel = sz
                views.append(flat[dt][off: off + numel].view(NPARTS[pr], *shape))
        wsq = sq[sq_off: sq_off + co * ci].view(co, ci) if want_wsq else None
        a = arr[k]
        a.weight = _ptr(w)
        a.image = views[0].data_ptr() if views[0] is not None else None
        a.image_t = views[1].data_ptr() if views[1] is not None else None
        a.wsq = _ptr(wsq)
        a.Cout, a.Cin, a.taps = co, ci, kh * kw
        a.precision = PRECISIONS[prec] if prec is not None else 0
        a.precision_t = PRECISIONS[prec_t] if prec_t is not None else 0
        for v in views:
            if v is not None and v.dtype == torch.float16:
                v.w_absmax = amax[k: k + 1]
                a.w_absmax = v.w_absmax.data_ptr()
        out.append((views[0], views[1], wsq))
    for k0 in range(0, len(items), 48):
        n = min(48, len(items) - k0)
        sub = (L.WeightPrepItem * n).from_buffer(arr, k0 * C.sizeof(L.WeightPrepItem))
        L.check(L.lib().hfagp_weight_prep_batch(sub, n, _stream()), "weight_prep_batch")
    return out


def weight_prep_split(weight: torch.Tensor, nparts: int) -> torch.Tensor:
    """The image of the RAW weight by part count (hfagp_weight_prep_split): 1 = 'f16' (a plain fp16 rounding of the weight: not
    scaled, so good for 2^-14 <= |w| <= 65504 only), 2 = 'bf16x3', 3 = 'bf16x6'."""
    return _weight_prep_prec(weight, {1: "f16", 2: "bf16x3", 3: "bf16x6"}[nparts], scaled=False)


def _style_args(a, who: str, w, affine_w, affine_b, wsq, style_gain: float, eps: float):
    """Fill the L.StyleArgs ``a`` of one layer; returns the outputs it points at: (styles [B, Cin], dcoef [B, Cout] | None)."""
    if w.dtype != torch.float32 or not w.is_cuda or w.stride(-1) != 1:
        raise RuntimeError(f"{who}: w must be a CUDA fp32 tensor with unit inner stride")
    if w.dim() != 2 or affine_w.dim() != 2:
        raise RuntimeError(f"{who}: w must be [B, w_dim] and affine_w [Cin, w_dim], got {list(w.shape)} and {list(affine_w.shape)}")
    b, wd = w.shape
    cin = affine_w.shape[0]
    _chk_operand(who, "affine_w", affine_w, (cin, wd), w)
    _chk_operand(who, "affine_b", affine_b, (cin,), w)
    if wsq is not None:
        if wsq.dim() != 2:
            raise RuntimeError(f"{who}: wsq must be [Cout, Cin], got {list(wsq.shape)}")
        _chk_operand(who, "wsq", wsq, (wsq.shape[0], cin), w)
    styles = torch.empty(b, cin, device=w.device, dtype=torch.float32)
    dcoef = None
    a.w, a.affine_w, a.affine_b = _ptr(w), _ptr(affine_w), _ptr(affine_b)
    a.styles = _ptr(styles)
    a.B, a.w_dim, a.w_stride, a.Cin = b, wd, w.stride(0), cin
    a.style_gain, a.eps = style_gain, eps
    if wsq is not None:
        dcoef = torch.empty(b, wsq.shape[0], device=w.device, dtype=torch.float32)
        a.wsq, a.dcoef, a.Cout = _ptr(wsq), _ptr(dcoef), wsq.shape[0]
    return styles, dcoef


def styles_demod(w: torch.Tensor, affine_w: torch.Tensor, affine_b: torch.Tensor,
                 wsq: Optional[torch.Tensor], style_gain: float = 1.0, eps: float = 1e-8):
    """w [B, w_dim] (may be a strided row view of ws) → styles [B, Cin], dcoef [B, Cout] | None."""
    a = L.StyleArgs()
    out = _style_args(a, "styles_demod", w, affine_w, affine_b, wsq, style_gain, eps)
    L.check(L.lib().hfagp_style_fwd(C.byref(a), _stream()), "style_fwd")
    return out


def styles_demod_batch(items):
    """``items``: sequence of (w [B, w_dim] row view, affine_w, affine_b, wsq | None, style_gain, eps), at most 32.
    One launch for all the styles, one for all the demodulation coefficients.  Returns [(styles, dcoef | None)]."""
    arr = (L.StyleArgs * len(items))()
    out = [_style_args(a, "styles_demod_batch", *item) for a, item in zip(arr, items)]
    L.check(L.lib().hfagp_style_batch_fwd(arr, len(items), _stream()), "style_batch_fwd")
    return out


def qr_gram(gram: torch.Tensor, top: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """gram = A^T A [n, n], top = A[:n, :n] → (R with LAPACK's signs, R^-1); Q = A @ R^-1 (n <= 64)."""
    n = gram.shape[0]
    r = torch.empty(n, n, device=gram.device, dtype=torch.float32)
    rinv = torch.empty(n, n, device=gram.device, dtype=torch.float32)
    L.check(L.lib().hfagp_qr_gram_fwd(_ptr(_chk(gram, "gram")), _ptr(_chk(top, "top")), _ptr(r), _ptr(rinv), n, _stream()),
            "qr_gram_fwd")
    return r, rinv


def qr_refine(gram: torch.Tensor, status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gram = Q1^T Q1 [n, n] → (upper Cholesky factor R2 with positive diagonal, R2^-1); status [2] (optional)
    receives (max |gram - I|, breakdown flag).  See include/hfagp.h."""
    n = gram.shape[0]
    r = torch.empty(n, n, device=gram.device, dtype=torch.float32)
    rinv = torch.empty(n, n, device=gram.device, dtype=torch.float32)
    L.check(L.lib().hfagp_qr_refine_fwd(_ptr(_chk(gram, "gram")), _ptr(r), _ptr(rinv), _ptr(status), n, _stream()),
            "qr_refine_fwd")
    return r, rinv


def tall_gram(x: torch.Tensor, y: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """scale * x^T y [n, n] for tall-skinny fp32 matrices [m, n <= 64], row- or column-major views (hfagp_tall_gram)."""
    m, n = x.shape
    for t in (x, y):
        if t.shape != (m, n) or t.dtype != torch.float32 or not t.is_cuda or 1 not in (t.stride(0), t.stride(1)):
            raise RuntimeError("tall_gram: operands must be fp32 device matrices of one shape with a unit stride")
    out = torch.empty(n, n, device=x.device, dtype=torch.float32)
    ws = torch.empty(L.lib().hfagp_tall_gram_workspace_bytes(m, n) // 4, device=x.device, dtype=torch.float32)
    L.check(L.lib().hfagp_tall_gram(x.data_ptr(), x.stride(0), x.stride(1), y.data_ptr(), y.stride(0), y.stride(1), _ptr(ws),
                                    _ptr(out), m, n, scale, _stream()), "tall_gram")
    return out


class TallSkinnyQR(torch.autograd.Function):
    """Q of the reduced QR of a tall-skinny fp32 CUDA matrix A [m, n <= 64] with torch.linalg.qr's (LAPACK's) sign
    convention; backward = the standard QR adjoint for dR = 0:
        dA = (dQ + Q S) R^-T,   X = triu(-Q^T dQ),   S = X + X^T - diag(X).
    Two passes: the Gram-matrix Householder kernel (Q1 = A R1^-1, orthogonality defect ~cond(A)^2 eps) and one
    Cholesky re-orthogonalisation of Q1 (Q = Q1 R2^-1, defect O(eps) while cond(A)^2 eps < ~0.3); R^-1 = R1^-1 R2^-1.
    `status` (device float[2], optional) receives the defect of pass 1 and the breakdown flag (ops.qr_refine)."""

    @staticmethod
    def forward(ctx, a: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
        n = a.shape[1]
        gram = tall_gram(a, a)
        _, rinv1 = qr_gram(gram, a[:n, :n].contiguous())
        q1 = a @ rinv1
        _, rinv2 = qr_refine(tall_gram(q1, q1), status)
        rinv = rinv1 @ rinv2
        q = q1 @ rinv2
        ctx.save_for_backward(q, rinv)
        return q

    @staticmethod
    def backward(ctx, gq: torch.Tensor):
        q, rinv = ctx.saved_tensors
        if gq.stride(0) != 1 and gq.stride(1) != 1:
            gq = gq.contiguous()
        x = torch.triu(tall_gram(q, gq, -1.0))
        s = x + x.T - torch.diag(torch.diagonal(x))
        return (gq + q @ s) @ rinv.T, None


def fully_connected(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], lr_mul: float = 1.0,
                    act: str = "linear", alpha: float = 0.2, gain: Optional[float] = None) -> torch.Tensor:
    """EG3D FullyConnectedLayer: act((x @ (W*lr_mul/sqrt(in)).T + b*lr_mul)) * gain."""
    _chk(x, "x")
    b, fin = x.shape
    fout = weight.shape[0]
    if gain is None:
        gain = math.sqrt(2.0) if act == "lrelu" else 1.0
    y = torch.empty(b, fout, device=x.device, dtype=torch.float32)
    L.check(L.lib().hfagp_fc_fwd(_ptr(x), _ptr(_chk(weight, "weight")), _ptr(bias), _ptr(y), b, fin, fout, lr_mul,
                                 _ACT[act], alpha, gain, _stream()), "fc_fwd")
    return y


# ----------------------------------------------------------------------------- modulated conv
def absmax_slots(n: int, device) -> torch.Tensor:
    """[n, 64 * 32] zeroed slot buffers (64 slots, one 128-byte line each) for the fp16 range tracking of n tensors (row i: max |.| of tensor i = row.max())."""
    return torch.zeros(n, L.ABSMAX_FLOATS, device=device, dtype=torch.float32)


_IMAGE_PRECISION = {(torch.float16, 1): PREC_F16, (torch.float16, 2): PREC_F16X3,
                    (torch.bfloat16, 2): PREC_BF16X3, (torch.bfloat16, 3): PREC_BF16X6}


def _image_precision(wt: torch.Tensor, x_parts: int = 0, who: str = "modconv") -> int:
    """PREC_* of a weight image: the fp32 image of `weight_prep`, or the 16-bit kind that dtype and part count of a
    `weight_prep_prec` image say; ``x_parts=1`` turns the two-part float16 image into 'f16x2' (see `modconv`)."""
    if wt.dtype == torch.float32:
        return PREC_F32
    prec = _IMAGE_PRECISION.get((wt.dtype, wt.shape[0])) if wt.dim() == 5 else None
    if prec is None:
        raise RuntimeError(f"{who}: 16-bit weight images must come from weight_prep_prec")
    if x_parts == 1 and prec != PREC_F16:
        if prec != PREC_F16X3:
            raise RuntimeError(f"{who}: x_parts=1 ('f16x2') goes with the two-part float16 weight image")
        prec = PREC_F16X2
    return prec


def _modconv_args(x: torch.Tensor, wt: torch.Tensor, cout: int, mode: int, styles=None, dcoef=None, noise=None,
                  noise_strength: float = 0.0, bias=None, act: str = "linear", alpha: float = 0.2, gain: float = 1.0,
                  clamp: Optional[float] = None, batch: Optional[int] = None, ksplit: int = 0, x_absmax=None, y_absmax=None,
                  rgb_w=None, y_f16: bool = False, x_parts: int = 0, who: str = "modconv"):
    """The L.ModconvArgs of one call, everything but the buffers the caller allocates (y, workspace, rgb_part), and (B, H, W).
    Launches and the questions put to the library about them (`_plan_unsplit`, `_fir_scratch_bytes`) are all built here."""
    if mode == CONVS2_BWD:                      # x = four parity images [2,2,B,H+1,W+1,Cin]
        _, _, xb, h, w, cin = x.shape
        h, w = h - 1, w - 1
    else:
        xb, h, w, cin = x.shape
    b = batch if batch is not None else xb
    a = L.ModconvArgs()
    a.x, a.wt, a.precision = x.data_ptr(), wt.data_ptr(), _image_precision(wt, x_parts, who)
    a.styles, a.dcoef, a.noise, a.bias = _ptr(styles), _ptr(dcoef), _ptr(noise), _ptr(bias)
    a.x_batch_stride = 0 if (xb == 1 and b > 1) else x.shape[-3] * x.shape[-2] * cin      # 0: one input broadcast over the batch
    a.B, a.H, a.W, a.Cin, a.Cout = b, h, w, cin, cout
    a.mode, a.act, a.ksplit = mode, _ACT[act], ksplit
    a.noise_strength, a.alpha, a.gain, a.clamp = noise_strength, alpha, gain, _clamp(clamp)
    a.x_absmax, a.y_absmax, a.rgb_w = _ptr(x_absmax), _ptr(y_absmax), _ptr(rgb_w)
    a.x_f16, a.y_f16 = int(x.dtype == torch.float16), int(y_f16)
    a.w_absmax = _ptr(getattr(wt, "w_absmax", None))              # a scaled float16 image (`weight_prep_prec`) brings max |w| along
    return a, b, h, w


def modconv(x: torch.Tensor, wt: torch.Tensor, cout: int, mode: int, styles: Optional[torch.Tensor] = None,
            dcoef: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, noise_strength: float = 0.0,
            bias: Optional[torch.Tensor] = None, act: str = "linear", alpha: float = 0.2, gain: float = 1.0,
            clamp: Optional[float] = None, batch: Optional[int] = None, ksplit: int = 0, x_absmax: Optional[torch.Tensor] = None,
            y_absmax: Optional[torch.Tensor] = None, rgb_w: Optional[torch.Tensor] = None, y_f16: bool = False,
            store_y: bool = True, x_parts: int = 0):
    """x [B|1, H, W, Cin] channels-last.  mode CONV3X3 / CONV1X1: fused epilogue, returns [B,H,W,Cout];
    mode CONVT3X3_UP2: returns the RAW transposed-conv result [B, 2H+1, 2W+1, Cout].
    ``wt`` from :func:`weight_prep` (fp32, exact MFMA) or :func:`weight_prep_split` (bfloat16 parts: the
    split-bf16 MFMA path, BF16X3 for 2 parts, BF16X6 for 3; float16, 1 part: the single-pass fp16 path).
    ``x_absmax`` / ``y_absmax`` ([64 x 32] fp32, `absmax_slots`): fp16 range tracking — max |x| of the input as published by its
    producer (the fp16 kinds scale the operand by an exact power of two so nothing saturates) and the slot buffer that
    receives max |y| of a fused-epilogue output (include/hfagp.h).
    ``rgb_w`` [B, 3, Cout] (toRGB weight x its styles): fused toRGB — returns (y, rgb_part [parts, B, H, W, 4]) for
    `torgb_finish`; only where `fused_torgb_supported` says so.  ``store_y=False`` (with rgb_w): y is not written and None
    is returned in its place (last super-resolution layer of a forward-only call).
    ``x_parts=1`` with the two-part float16 image: precision 'f16x2' — the activations as ONE fp16 part against the 22-bit
    weights, two MFMAs per product (TF32 class; include/hfagp.h HFAGP_PREC_F16X2).
    fp16 STORAGE (single-pass fp16 weights only, `f16_storage_supported`): a float16 ``x`` is read as stored and
    ``y_f16`` writes the result as float16 (EG3D's fp16 super-resolution blocks keep their activations in fp16)."""
    if (x.dtype == torch.float16 or y_f16) and not (wt.dtype == torch.float16 and wt.dim() == 5 and wt.shape[0] == 1):
        raise RuntimeError("modconv: fp16 storage (float16 x / y_f16) goes with the single-pass fp16 weight image")
    _chk_act(x, "x")
    if wt.dtype == torch.float32:
        _chk(wt, "wt")
    elif not (wt.is_cuda and wt.is_contiguous()):
        raise RuntimeError("modconv: 16-bit weight images must come from weight_prep_prec")
    if rgb_w is not None:
        _chk(rgb_w, "rgb_w")
    # (rgb_w is in the args BEFORE the workspace query: the kernel choice — small-image vs staged — reads it)
    a, b, h, w = _modconv_args(x, wt, cout, mode, styles, dcoef, noise, noise_strength, bias, act, alpha, gain, clamp, batch,
                               ksplit, x_absmax, y_absmax, rgb_w, y_f16, x_parts)
    ydt = torch.float16 if y_f16 else torch.float32
    if not store_y:                             # only the fused toRGB sums are wanted (`rgb_w`): the activation is not written at all
        if rgb_w is None or y_absmax is not None:
            raise RuntimeError("modconv: store_y=False needs rgb_w (the fused toRGB is then the only output) and no y_absmax")
        y = None
    elif mode == CONVT3X3_UP2:
        y = torch.empty(b, 2 * h + 1, 2 * w + 1, cout, device=x.device, dtype=ydt)
    else:
        y = torch.empty(b, h, w, cout, device=x.device, dtype=ydt)
    a.y = _ptr(y)
    nbytes = L.lib().hfagp_modconv_workspace_bytes(C.byref(a))
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32) if nbytes else None
    part = None
    if rgb_w is not None:
        part = torch.empty(L.lib().hfagp_modconv_rgb_parts(C.byref(a)), b, h, w, 4, device=x.device, dtype=torch.float32)
    a.workspace, a.rgb_part = _ptr(ws), _ptr(part)
    L.check(L.lib().hfagp_modconv_fwd(C.byref(a), _stream()), "modconv_fwd")
    return y if rgb_w is None else (y, part)


_PLAN_UNSPLIT = {}       # (mode, B, H, W, Cin, Cout, precision, x_f16, y_f16, fused toRGB, broadcast x) -> hfagp_modconv_workspace_bytes() == 0
_NONNULL = 1             # stands in for a buffer that does not exist yet when the library is only ASKED about a call


def _plan_unsplit(key, build, rgb: bool = False) -> bool:
    """Whether the library runs the call ``build()`` describes (`_modconv_args`; ``rgb``: with a fused toRGB) WITHOUT splitting K,
    the epilogue in the conv kernel: hfagp_modconv_workspace_bytes() == 0 (include/hfagp.h), asked once per ``key`` (the fields
    of the call that planning reads).  The plan's developer switches are not in the key: the library reads them once per process
    (`static` in make_plan, csrc/modconv_plan.h).  Planning dereferences nothing, but wants x / wt / y (and rgb_w) non-null."""
    r = _PLAN_UNSPLIT.get(key)
    if r is None:
        a = build()
        a.x, a.wt, a.y, a.rgb_w = a.x or _NONNULL, a.wt or _NONNULL, _NONNULL, _NONNULL if rgb else None
        r = _PLAN_UNSPLIT[key] = L.lib().hfagp_modconv_workspace_bytes(C.byref(a)) == 0
    return r


def f16_storage_supported(h: int, w: int, cin: int, cout: int, batch: int) -> bool:
    """Whether a 3x3 AND an up-sampling modconv on an h x w input grid can keep their activations in fp16 (`modconv` y_f16,
    float16 x): Cin a multiple of 16, 128-channel output tiles, and launches the library does not split along K — its own
    answer (`_plan_unsplit`) for the two calls, described here from their shapes alone."""
    if cin % 16 != 0 or cout % 128 != 0:
        return False

    def call(mode):
        x = torch.empty(batch, h, w, cin, dtype=torch.float16, device="meta")
        wt = torch.empty(1, 9, cin // 8, cout, 8, dtype=torch.float16, device="meta")      # (`weight_prep_prec(.., "f16")`)
        return _modconv_args(x, wt, cout, mode, y_f16=True)[0]
    return all(_plan_unsplit((mode, batch, h, w, cin, cout, PREC_F16, 1, 1, False, False), lambda: call(mode))
               for mode in (CONV3X3, CONVT3X3_UP2))


def fused_torgb_supported(x: torch.Tensor, wt: torch.Tensor, cout: int, batch: int) -> bool:
    """Whether `modconv(..., mode=CONV3X3, rgb_w=...)` can form the toRGB sums in its epilogue: 16-bit weight image,
    Cout a multiple of 128, and a launch the library does not split along K (then the epilogue lives in the reducer): its
    own answer for that call (`_plan_unsplit`)."""
    if wt.dtype == torch.float32 or cout % 128 != 0:
        return False
    xb, h, w, cin = x.shape
    key = (CONV3X3, batch, h, w, cin, cout, _image_precision(wt), int(x.dtype == torch.float16), 0, True, xb == 1 and batch > 1)
    return _plan_unsplit(key, lambda: _modconv_args(x, wt, cout, CONV3X3, batch=batch)[0], rgb=True)


def torgb_finish(part: torch.Tensor, bias: torch.Tensor, rgb_in: Optional[torch.Tensor], clamp: Optional[float],
                 y_pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rgb_part of a fused-toRGB conv -> NCHW image: clamp(sum of parts + bias) + upsample2d(rgb_in)."""
    _chk(part, "part")
    if part.dim() != 5 or part.shape[4] != 4 or bias.dim() != 1:
        raise RuntimeError(f"torgb_finish: part must be [nparts, B, H, W, 4] and bias [Cout], got {list(part.shape)} and {list(bias.shape)}")
    nparts, b, h, w, _ = part.shape
    cout = bias.shape[0]
    _chk_operand("torgb_finish", "bias", bias, (cout,), part)
    _chk_operand("torgb_finish", "rgb_in", rgb_in, (b, cout, h // 2, w // 2), part)
    _chk_operand("torgb_finish", "y_pre", y_pre, (b, cout, h, w), part)
    out = torch.empty(b, cout, h, w, device=part.device, dtype=torch.float32)
    a = L.TorgbFinishArgs()
    a.part, a.bias, a.rgb_out, a.y_pre = _ptr(part), _ptr(bias), _ptr(out), _ptr(y_pre)
    a.rgb_in = _ptr(rgb_in)
    a.nparts, a.B, a.H, a.W, a.Cout = nparts, b, h, w, cout
    a.clamp = _clamp(clamp)
    L.check(L.lib().hfagp_torgb_finish_fwd(C.byref(a), _stream()), "torgb_finish_fwd")
    return out


_FIR_SCRATCH = {}        # (device, stream) -> scratch tensor of upconv_fir, grown on demand to the next power of two
_FIR_RETIRED = []        # outgrown scratch tensors stay alive: a HIP graph captured earlier may still replay against them
_FIR_BYTES = {}          # (shape, precision, storage, developer switches) -> hfagp_upconv_fir_scratch_bytes (0 = not supported)


def _fir_scratch_bytes(a) -> int:
    """hfagp_upconv_fir_scratch_bytes, memoised per layer shape: the library builds the whole launch plan to answer, and the
    generator asks twice per up-sampling layer call (supported? / how much scratch?)."""
    key = (a.B, a.H, a.W, a.Cin, a.Cout, a.precision, a.x_f16, a.x_batch_stride == 0,
           os.environ.get("HFAGP_DEV_FIR_MIN_BLOCKS"), os.environ.get("HFAGP_DEV_FIR_NSEG"), os.environ.get("HFAGP_DEV_FIR_LEAN"))
    n = _FIR_BYTES.get(key)
    if n is None:
        n = _FIR_BYTES[key] = int(L.lib().hfagp_upconv_fir_scratch_bytes(C.byref(a)))
    return n


def upconv_fir_supported(x: torch.Tensor, wt: torch.Tensor, cout: int, batch: Optional[int] = None) -> bool:
    """Whether `upconv_fir` takes this up-sampling layer (16-bit weight image with one or two parts, Cin % 16 == 0,
    Cout % 128 == 0 and a launch that fills the chip): the library's own rule, hfagp_upconv_fir_scratch_bytes() > 0."""
    if wt.dtype == torch.float32 or not x.is_cuda or (x.dtype == torch.float16 and not (wt.dtype == torch.float16 and wt.shape[0] == 1)):
        return False
    a, *_ = _modconv_args(x, wt, cout, CONVT3X3_UP2, batch=batch, who="upconv_fir")
    return _fir_scratch_bytes(a) > 0


def upconv_fir(x: torch.Tensor, wt: torch.Tensor, cout: int, styles: Optional[torch.Tensor], dcoef: Optional[torch.Tensor],
               noise: Optional[torch.Tensor], noise_strength: float, bias: Optional[torch.Tensor], act: str = "lrelu",
               alpha: float = 0.2, gain: float = math.sqrt(2.0), clamp: Optional[float] = None, batch: Optional[int] = None,
               x_absmax: Optional[torch.Tensor] = None, y_absmax: Optional[torch.Tensor] = None,
               y_f16: bool = False) -> torch.Tensor:
    """The up-sampling layer of a synthesis block in one pass: x [B|1, H, W, Cin] -> [B, 2H, 2W, Cout] =
    bias_act(FIR(conv_transpose2d(x * styles, W, stride 2)) * dcoef + noise) (EG3D conv2d_resample(up=2) + bias_act), the raw
    transposed-conv result never leaving the chip (`modconv(mode=CONVT3X3_UP2)` + `upfir_epilogue` move it through HBM in
    fp32).  Only where `upconv_fir_supported` says so."""
    _chk_act(x, "x")
    if wt.dtype == torch.float32 or not (wt.is_cuda and wt.is_contiguous() and wt.dim() == 5):
        raise RuntimeError("upconv_fir: needs a 16-bit weight image from weight_prep_prec")
    a, b, h, w = _modconv_args(x, wt, cout, CONVT3X3_UP2, styles, dcoef, noise, noise_strength, bias, act, alpha, gain, clamp,
                               batch, x_absmax=x_absmax, y_absmax=y_absmax, y_f16=y_f16, who="upconv_fir")
    nbytes = _fir_scratch_bytes(a)
    if nbytes == 0:
        raise RuntimeError("upconv_fir: this layer shape / precision / batch is not supported (upconv_fir_supported)")
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    scratch = _FIR_SCRATCH.get(key)
    if scratch is None or scratch.numel() * 4 < nbytes:
        if scratch is not None:
            _FIR_RETIRED.append(scratch)
        grown = 1 << max(nbytes - 1, 1).bit_length()           # powers of two: a handful of growth steps per process at most
        scratch = _FIR_SCRATCH[key] = torch.empty(grown // 4, device=x.device, dtype=torch.float32)
    y = torch.empty(b, 2 * h, 2 * w, cout, device=x.device, dtype=torch.float16 if y_f16 else torch.float32)
    a.y = y.data_ptr()
    L.check(L.lib().hfagp_upconv_fir_fwd(C.byref(a), _ptr(scratch), _stream()), "upconv_fir_fwd")
    return y


def upfir_epilogue(yt: torch.Tensor, dcoef: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                   noise_strength: float, bias: Optional[torch.Tensor], act: str = "lrelu", alpha: float = 0.2,
                   gain: float = math.sqrt(2.0), clamp: Optional[float] = None,
                   y_absmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """yt [B, 2H+1, 2W+1, C] raw transposed conv → FIR(pad 1, gain 4) → demod/noise/bias/act → [B,2H,2W,C].
    A float16 ``yt`` (fp16 storage, `modconv` y_f16) gives a float16 result; the arithmetic is fp32 either way.
    ``y_absmax`` (`absmax_slots`) receives max |result| of the values as stored."""
    half = _chk_act(yt, "yt").dtype == torch.float16
    if yt.dim() != 4 or yt.shape[1] < 3 or yt.shape[2] < 3 or yt.shape[1] % 2 == 0 or yt.shape[2] % 2 == 0:
        raise RuntimeError(f"upfir_epilogue: yt must be [B, 2H+1, 2W+1, C] with an odd height and width of at least 3, got {list(yt.shape)}")
    b, hi, wi, c = yt.shape
    h, w = (hi - 1) // 2, (wi - 1) // 2
    _chk_operand("upfir_epilogue", "dcoef", dcoef, (b, c), yt)
    _chk_operand("upfir_epilogue", "noise", noise, (2 * h, 2 * w), yt)
    _chk_operand("upfir_epilogue", "bias", bias, (c,), yt)
    _chk_absmax("upfir_epilogue", "y_absmax", y_absmax, yt)
    y = torch.empty(b, 2 * h, 2 * w, c, device=yt.device, dtype=yt.dtype)
    a = L.UpfirEpilogueArgs()
    a.yt, a.dcoef, a.noise, a.bias, a.y = yt.data_ptr(), _ptr(dcoef), _ptr(noise), _ptr(bias), y.data_ptr()
    a.io_f16 = int(half)
    a.B, a.H, a.W, a.C, a.act = b, h, w, c, _ACT[act]
    a.noise_strength, a.alpha, a.gain = noise_strength, alpha, gain
    a.clamp = _clamp(clamp)
    a.y_absmax = _ptr(y_absmax)
    L.check(L.lib().hfagp_upfir_epilogue_fwd(C.byref(a), _stream()), "upfir_epilogue_fwd")
    return y


def skip_upsample_add(img: Optional[torch.Tensor], y: torch.Tensor, plane_major: bool = False,
                      out_absmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SynthesisBlock 'skip': upsample2d(img) + y (channels-last).  plane_major → [B,3,H,W,C/3].  out_absmax ([64 x 32],
    `absmax_slots`): receives max |output| (the bound the ray marcher's 16-bit decoder scales by)."""
    _chk(y, "y")
    if y.dim() != 4:
        raise RuntimeError(f"skip_upsample_add: y must be [B, H, W, C], got {list(y.shape)}")
    b, ho, wo, c = y.shape
    _chk_absmax("skip_upsample_add", "out_absmax", out_absmax, y)
    a = L.SkipArgs()
    if img is not None:
        if ho % 2 or wo % 2:
            raise RuntimeError(f"skip_upsample_add: y {list(y.shape)} must have an even height and width to add an up-sampled img to")
        _chk_operand("skip_upsample_add", "img", img, (b, ho // 2, wo // 2, c), y)
        a.img_in, a.H, a.W = _ptr(img), img.shape[1], img.shape[2]
    else:
        a.H, a.W = ho, wo
    out = torch.empty((b, 3, ho, wo, c // 3) if plane_major else (b, ho, wo, c), device=y.device,
                      dtype=torch.float32)
    a.y, a.img_out, a.B, a.C, a.plane_major = _ptr(y), _ptr(out), b, c, int(plane_major)
    a.out_absmax = _ptr(out_absmax)
    L.check(L.lib().hfagp_skip_upsample_add(C.byref(a), _stream()), "skip_upsample_add")
    return out


def torgb_skip_supported(x: torch.Tensor, wt: torch.Tensor, cout: int) -> bool:
    """Whether `torgb_skip` (hfagp_torgb_skip_fwd, the streaming toRGB + skip kernel) takes this layer: a 16-bit weight
    image, Cout a multiple of 32 (<= 128), Cin a multiple of 16 (<= 512), rows of a multiple of 32 positions, and enough
    positions to fill the chip."""
    b, h, w, cin = x.shape
    # (below 512 wave tiles of 32 positions the K loop's HBM latency is not covered by other waves — at one frame the
    # 32^2 and 64^2 blocks take 46 / 42 us here against 24 / 27 us for the split-K conv + reducer + skip kernels)
    return (wt.dtype in (torch.float16, torch.bfloat16) and cout % 32 == 0 and cout <= 128 and cin % 16 == 0 and
            cin <= 512 and w % 32 == 0 and (h * w) % 128 == 0 and b * h * w >= 512 * 32)


def torgb_skip(x: torch.Tensor, wt: torch.Tensor, cout: int, styles: torch.Tensor, bias: torch.Tensor,
               img: Optional[torch.Tensor], plane_major: bool = False, x_absmax: Optional[torch.Tensor] = None,
               out_absmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SynthesisBlock 'skip' branch in one pass: upsample2d(img) + toRGB(x) (1x1 modulated conv, linear, bias), x and img
    channels-last; returns [B,H,W,Cout] or, plane_major, [B,3,H,W,Cout/3].  ``wt``: `weight_prep_prec` image of the toRGB
    weight.  Same bits as `modconv(CONV1X1)` + `skip_upsample_add` (when that conv is not split along K)."""
    _chk(x, "x")
    b, h, w, cin = x.shape
    if not (wt.is_cuda and wt.is_contiguous() and wt.dim() == 5 and wt.dtype in (torch.float16, torch.bfloat16)):
        raise RuntimeError("torgb_skip: the weight image must come from weight_prep_prec (16-bit kinds)")
    a = L.TorgbSkipArgs()
    a.precision = _image_precision(wt, who="torgb_skip")
    out = torch.empty((b, 3, h, w, cout // 3) if plane_major else (b, h, w, cout), device=x.device, dtype=torch.float32)
    a.x, a.wt, a.styles, a.bias = _ptr(x), wt.data_ptr(), _ptr(_chk(styles, "styles")), _ptr(_chk(bias, "bias"))
    if img is not None:
        _chk(img, "img")
        if img.shape != (b, h // 2, w // 2, cout):
            raise RuntimeError(f"torgb_skip: img {tuple(img.shape)} is not the half-resolution image of {(b, h, w, cout)}")
        a.img_in = _ptr(img)
    a.img_out, a.x_absmax, a.out_absmax = _ptr(out), _ptr(x_absmax), _ptr(out_absmax)
    a.w_absmax = _ptr(getattr(wt, "w_absmax", None))
    a.B, a.H, a.W, a.Cin, a.Cout, a.plane_major = b, h, w, cin, cout, int(plane_major)
    L.check(L.lib().hfagp_torgb_skip_fwd(C.byref(a), _stream()), "torgb_skip_fwd")
    return out


def torgb_small(x: torch.Tensor, weight: torch.Tensor, styles: torch.Tensor, bias: torch.Tensor,
                rgb_in: Optional[torch.Tensor], clamp: Optional[float], y_pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ToRGBLayer with ≤4 output channels + skip add; x channels-last, rgb NCHW.  `y_pre` (optional,
    [B,Cout,H,W]) receives the toRGB output before clamp and skip add (backward needs the clamp mask)."""
    _chk(x, "x")
    if x.dim() != 4 or weight.dim() != 2:
        raise RuntimeError(f"torgb_small: x must be [B, H, W, Cin] and weight [Cout, Cin], got {list(x.shape)} and {list(weight.shape)}")
    b, h, w, cin = x.shape
    cout = weight.shape[0]
    _chk_operand("torgb_small", "weight", weight, (cout, cin), x)
    _chk_operand("torgb_small", "styles", styles, (b, cin), x)
    _chk_operand("torgb_small", "bias", bias, (cout,), x)
    _chk_operand("torgb_small", "rgb_in", rgb_in, (b, cout, h // 2, w // 2), x)
    _chk_operand("torgb_small", "y_pre", y_pre, (b, cout, h, w), x)
    out = torch.empty(b, cout, h, w, device=x.device, dtype=torch.float32)
    a = L.TorgbArgs()
    a.y_pre = _ptr(y_pre)
    a.x, a.weight, a.styles, a.bias = _ptr(x), _ptr(weight), _ptr(styles), _ptr(bias)
    a.rgb_in = _ptr(rgb_in)
    a.rgb_out = _ptr(out)
    a.B, a.H, a.W, a.Cin, a.Cout = b, h, w, cin, cout
    a.clamp = _clamp(clamp)
    L.check(L.lib().hfagp_torgb_fwd(C.byref(a), _stream()), "torgb_fwd")
    return out


# ----------------------------------------------------------------------------- renderer
# The library sees pointers and integers, never a tensor's extent: these builders are the only guard between a mis-shaped tensor and
# a kernel that reads past it.  Every renderer entry point fills its structures through them and raises before anything is launched.
_DEC = ("dec_w0", "dec_b0", "dec_w1", "dec_b1")


def _planes_dims(who: str, planes: torch.Tensor):
    """(B, H, W) of channels-last tri-planes."""
    _chk(planes, f"{who}: planes")
    if planes.dim() != 5 or planes.shape[1] != 3 or planes.shape[4] != 32:
        raise RuntimeError(f"{who}: planes must be [B, 3, H, W, 32]")
    return planes.shape[0], planes.shape[2], planes.shape[3]


def _plane_axes_id(plane_axes) -> int:
    """The library's code of a plane-axes convention, given as that code or as the config's name."""
    if isinstance(plane_axes, str):
        return 0 if plane_axes == "eg3d_original" else 1
    return plane_axes


def _fill_decoder(who: str, a, planes: torch.Tensor, params, decoder_precision: str, planes_absmax) -> None:
    """The decoder's four parameter pointers and its |planes| bound, into a RaymarchArgs / PlanesQueryArgs / PlanesQueryBwdArgs.  A
    bound that `_decoder_bound` returned earlier passes through unchanged (`raymarch_bwd`: one for all frame chunks)."""
    for name, t in zip(_DEC, params):
        setattr(a, name, _ptr(_chk(t, f"{who}: {name}")))
    # (no frames: nothing is launched that could read a bound, and there is nothing to reduce over)
    a.planes_absmax = _ptr(_decoder_bound(planes, decoder_precision, planes_absmax)) if planes.numel() else None


def _ray_args(who: str, f, planes, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1, res: int, ray_start: float,
              ray_end: float, box_warp: float, decoder_lr_mul: float, plane_axes, white_back: bool, decoder_precision: str, planes_absmax,
              state):
    """Fills the RaymarchArgs ``f`` (a fresh one, or the `fwd` member of a RaymarchBwdArgs) with everything but the forward's output
    pointers, and returns (B, H, W, R, Sc, Sf).  Owns the checks of planes, the uniforms' element counts, `state` and of device,
    dtype and contiguity of every input.  The parameters after ``f`` are `raymarch`'s, in its order."""
    b, h, w = _planes_dims(who, planes)
    r = res * res
    sc, sf = u_strat.shape[-1], u_imp.shape[-1]
    if u_strat.numel() != b * r * sc or u_imp.numel() != b * r * sf:
        raise RuntimeError(f"{who}: u_strat / u_imp have the wrong number of elements")
    if state is not None and _chk(state, f"{who}: state").shape != (b, r, (sc + sf) * 35):
        raise RuntimeError(f"{who}: state must be [B, R, {(sc + sf) * 35}] (raymarch_state), got {tuple(state.shape)}")
    for name, t in (("cam2world", cam2world), ("intrinsics", intrinsics), ("u_strat", u_strat), ("u_imp", u_imp)):
        setattr(f, name, _ptr(_chk(t, f"{who}: {name}")))
    _fill_scene(who, f, planes, state, (b, h, w, res, sc, sf), (dec_w0, dec_b0, dec_w1, dec_b1), ray_start, ray_end, box_warp,
                decoder_lr_mul, plane_axes, white_back, decoder_precision, planes_absmax)
    return b, h, w, r, sc, sf


def _fill_scene(who: str, f, planes, state, dims, dec, ray_start: float, ray_end: float, box_warp: float, decoder_lr_mul: float,
                plane_axes, white_back: bool, decoder_precision: str, planes_absmax):
    """What the RaymarchArgs ``f`` of a grid and of a list have in common: planes, state, the decoder ``dec`` with its bound,
    ``dims`` = (B, H, W, res, Sc, Sf) and the scalars."""
    f.planes, f.state = _ptr(planes), _ptr(state)
    _fill_decoder(who, f, planes, dec, decoder_precision, planes_absmax)
    f.B, f.H, f.W, f.res, f.Sc, f.Sf = dims
    f.plane_axes, f.white_back = _plane_axes_id(plane_axes), int(white_back)
    f.ray_start, f.ray_end, f.box_warp, f.decoder_lr_mul = ray_start, ray_end, box_warp, decoder_lr_mul


def _ray_list_args(who: str, l, planes, ray_origins, ray_directions, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1, ray_start: float,
                   ray_end: float, box_warp: float, decoder_lr_mul: float, plane_axes, white_back: bool, decoder_precision: str,
                   planes_absmax, state, t_near=None, t_far=None):
    """`_ray_args` for a ray list: fills the RayListArgs / RayListBwdArgs ``l`` — the rays, R, and its RaymarchArgs member but the
    camera (ignored by the list entry points) and the forward's outputs — and returns (B, H, W, R, Sc, Sf, limits).  Owns the checks
    of the rays' shapes, the uniforms' element counts, `state`, the per-ray limits and of device, dtype and contiguity of every
    input.  ``limits``: a filled RayLimits when t_near / t_far [B,R] are given (both or neither) — the caller then runs the
    `limits` entry point — else None."""
    f = l.base if isinstance(l, L.RayListArgs) else l.bwd.fwd
    b, h, w = _planes_dims(who, planes)
    for name, t in (("ray_origins", ray_origins), ("ray_directions", ray_directions)):
        if _chk(t, f"{who}: {name}").dim() != 3 or t.shape[0] != b or t.shape[2] != 3:
            raise RuntimeError(f"{who}: {name} must be [B={b}, R, 3], got {tuple(t.shape)}")
    if ray_origins.shape != ray_directions.shape:
        raise RuntimeError(f"{who}: ray_origins {tuple(ray_origins.shape)} and ray_directions {tuple(ray_directions.shape)} differ")
    r = ray_origins.shape[1]
    sc, sf = u_strat.shape[-1], u_imp.shape[-1]
    if u_strat.numel() != b * r * sc or u_imp.numel() != b * r * sf:
        raise RuntimeError(f"{who}: u_strat / u_imp have the wrong number of elements")
    if state is not None and _chk(state, f"{who}: state").shape != (b, r, (sc + sf) * 35):
        raise RuntimeError(f"{who}: state must be [B, R, {(sc + sf) * 35}] (raymarch_rays_state), got {tuple(state.shape)}")
    for name, t in (("u_strat", u_strat), ("u_imp", u_imp)):
        setattr(f, name, _ptr(_chk(t, f"{who}: {name}")))
    _fill_scene(who, f, planes, state, (b, h, w, 0, sc, sf), (dec_w0, dec_b0, dec_w1, dec_b1), ray_start, ray_end, box_warp,
                decoder_lr_mul, plane_axes, white_back, decoder_precision, planes_absmax)
    l.ray_origins, l.ray_directions, l.R = _ptr(ray_origins), _ptr(ray_directions), r
    if (t_near is None) != (t_far is None):
        raise RuntimeError(f"{who}: t_near and t_far go together (both or neither)")
    limits = None
    if t_near is not None:
        for name, t in (("t_near", t_near), ("t_far", t_far)):
            if _chk(t, f"{who}: {name}").shape != (b, r):
                raise RuntimeError(f"{who}: {name} must be [B, R] = [{b}, {r}], got {tuple(t.shape)}")
        limits = L.RayLimits()
        limits.t_near, limits.t_far = _ptr(t_near), _ptr(t_far)
    return b, h, w, r, sc, sf, limits


def _dec_grad_out(who: str, a, params, decoder_grads: bool, dec_out):
    """The four tensors the decoder-parameter gradients are ACCUMULATED into, their pointers set in the RaymarchBwdArgs /
    PlanesQueryBwdArgs ``a``: ``dec_out`` (the parameters' .grad slices, say) or fresh zeros; None without ``decoder_grads``."""
    if not decoder_grads:
        return None
    dec = tuple(dec_out) if dec_out is not None else tuple(torch.zeros_like(t) for t in params)
    if len(dec) != 4 or any(t.shape != like.shape or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda
                            for t, like in zip(dec, params)):
        raise RuntimeError(f"{who}: dec_out must be four contiguous fp32 device tensors shaped like the decoder parameters")
    a.d_dec_w0, a.d_dec_b0, a.d_dec_w1, a.d_dec_b1 = (_ptr(t) for t in dec)
    return dec


def _query_points(who: str, coords: torch.Tensor, b: int) -> int:
    """M of explicit query points [1 or B, M, 3]."""
    _chk(coords, f"{who}: coords")
    if coords.dim() != 3 or coords.shape[2] != 3 or coords.shape[0] not in (1, b):
        raise RuntimeError(f"{who}: coords must be [1 or B={b}, M, 3], got {tuple(coords.shape)}")
    return coords.shape[1]


def raymarch(planes: torch.Tensor, cam2world: torch.Tensor, intrinsics: torch.Tensor, u_strat: torch.Tensor,
             u_imp: torch.Tensor, dec_w0: torch.Tensor, dec_b0: torch.Tensor, dec_w1: torch.Tensor,
             dec_b1: torch.Tensor, res: int, ray_start: float, ray_end: float, box_warp: float,
             decoder_lr_mul: float = 1.0, plane_axes: int = 0, white_back: bool = False,
             decoder_precision: str = "f16x3", planes_absmax: Optional[torch.Tensor] = None,
             state: Optional[torch.Tensor] = None):
    """planes [B,3,H,W,32] → feat [B,R,32], depth [B,R] (unclamped), wsum [B,R], tminmax [B,R,2].
    ``state`` (`raymarch_state`): receives the per-sample colours / densities / depths / sort order of every ray, so that
    `raymarch_bwd` of the same step need not gather and decode every sample again for the compositing adjoint.
    decoder_precision 'f16x3': the decoder MLP on the 16-bit matrix pipe with split fp16 operands (fp32-class); it needs
    a bound on |planes| — `planes_absmax` (64 slots as published by `skip_upsample_add(out_absmax=...)`), computed here
    with one reduction over the planes when the caller has none.  'fp32': the exact fp32 matrix instructions."""
    a = L.RaymarchArgs()
    b, _, _, r, _, _ = _ray_args("raymarch", a, planes, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1, res, ray_start,
                                 ray_end, box_warp, decoder_lr_mul, plane_axes, white_back, decoder_precision, planes_absmax, state)
    dev = planes.device
    feat = torch.empty(b, r, 32, device=dev, dtype=torch.float32)
    depth = torch.empty(b, r, device=dev, dtype=torch.float32)
    wsum = torch.empty(b, r, device=dev, dtype=torch.float32)
    tmm = torch.empty(b, r, 2, device=dev, dtype=torch.float32)
    a.feat, a.depth, a.wsum, a.tminmax = _ptr(feat), _ptr(depth), _ptr(wsum), _ptr(tmm)
    L.check(L.lib().hfagp_raymarch_fwd(C.byref(a), _stream()), "raymarch_fwd")
    return feat, depth, wsum, tmm


def raymarch_rays(planes: torch.Tensor, ray_origins: torch.Tensor, ray_directions: torch.Tensor, u_strat: torch.Tensor,
                  u_imp: torch.Tensor, dec_w0: torch.Tensor, dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor,
                  ray_start: float, ray_end: float, box_warp: float, decoder_lr_mul: float = 1.0, plane_axes: int = 0,
                  white_back: bool = False, decoder_precision: str = "f16x3", planes_absmax: Optional[torch.Tensor] = None,
                  state: Optional[torch.Tensor] = None, t_near: Optional[torch.Tensor] = None,
                  t_far: Optional[torch.Tensor] = None, samples: bool = False):
    """`raymarch` on caller-given rays: ray_origins / ray_directions [B,R,3] (directions as given, not normalised: a sample is
    o + t d) instead of (cam2world, intrinsics, res) → feat [B,R,32], depth [B,R] (unclamped), wsum [B,R], tminmax [B,R,2].
    u_strat [B,R,Sc], u_imp [B*R,Sf]; ``state``: `raymarch_rays_state`.  Everything else as `raymarch`.
    ``t_near`` / ``t_far`` [B,R] (both or neither; `ray_limits_box`, or any limits of the caller's): every ray is sampled on its own
    interval instead of [ray_start, ray_end], which is then ignored (hfagp_raymarch_rays_limits_fwd).  A ray whose limits are not
    finite or have far <= near is EMPTY and not marched: feat = the background (−1, or +1 with white_back), wsum 0, depth +inf,
    tminmax (+inf, −inf) — `depth_range(..., empty_rays=True)` / `depth_clamp_(..., empty_rays=True)` take such a call.
    ``samples``: two more results (hfagp_raymarch_rays_samples_fwd) — sample_weights [B,R,Sc+Sf−1], the compositing weight
    w_e = α_e·T_e of the interval between sorted samples e and e+1 (the values the kernel composites with: their sum is wsum), and
    sample_depths [B,R,Sc+Sf], ascending; both zero for an empty ray.  The other four results keep their bits."""
    a = L.RayListArgs()
    b, _, _, r, sc, sf, lim = _ray_list_args("raymarch_rays", a, planes, ray_origins, ray_directions, u_strat, u_imp, dec_w0, dec_b0,
                                             dec_w1, dec_b1, ray_start, ray_end, box_warp, decoder_lr_mul, plane_axes, white_back,
                                             decoder_precision, planes_absmax, state, t_near, t_far)
    dev = planes.device
    feat = torch.empty(b, r, 32, device=dev, dtype=torch.float32)
    depth = torch.empty(b, r, device=dev, dtype=torch.float32)
    wsum = torch.empty(b, r, device=dev, dtype=torch.float32)
    tmm = torch.empty(b, r, 2, device=dev, dtype=torch.float32)
    out = (feat, depth, wsum, tmm)
    if samples:
        so = L.RaySamples()
        out += (torch.empty(b, r, sc + sf - 1, device=dev, dtype=torch.float32), torch.empty(b, r, sc + sf, device=dev, dtype=torch.float32))
        so.weights, so.depths = _ptr(out[4]), _ptr(out[5])
    if b * r == 0:
        return out
    f = a.base
    f.feat, f.depth, f.wsum, f.tminmax = _ptr(feat), _ptr(depth), _ptr(wsum), _ptr(tmm)
    if samples:
        L.check(L.lib().hfagp_raymarch_rays_samples_fwd(C.byref(a), C.byref(lim) if lim is not None else None, C.byref(so), _stream()),
                "raymarch_rays_samples_fwd")
        return out
    if lim is not None:
        L.check(L.lib().hfagp_raymarch_rays_limits_fwd(C.byref(a), C.byref(lim), _stream()), "raymarch_rays_limits_fwd")
    else:
        L.check(L.lib().hfagp_raymarch_rays_fwd(C.byref(a), _stream()), "raymarch_rays_fwd")
    return feat, depth, wsum, tmm


def ray_limits_box(ray_origins: torch.Tensor, ray_directions: torch.Tensor, box_side: float):
    """(t_near, t_far), each [B,R]: every ray's slab intersection with the cube [−box_side/2, box_side/2]³ the tri-planes cover
    (box_side = cfg.box_warp) — EG3D's ray_start = ray_end = 'auto' — for `raymarch_rays(..., t_near=, t_far=)`.  t_near is clamped
    below at 0 (an origin inside the cube starts at the origin); a ray that misses has t_far <= t_near, a 0 · inf case gives NaN
    limits: both are empty rays to the ray marcher.  One launch (hfagp_ray_limits_box); `cam_utils.ray_limits_box` is the same
    formula in torch."""
    who = "ray_limits_box"
    for name, t in (("ray_origins", ray_origins), ("ray_directions", ray_directions)):
        if _chk(t, f"{who}: {name}").dim() != 3 or t.shape[2] != 3:
            raise RuntimeError(f"{who}: {name} must be [B, R, 3], got {tuple(t.shape)}")
    if ray_origins.shape != ray_directions.shape:
        raise RuntimeError(f"{who}: ray_origins {tuple(ray_origins.shape)} and ray_directions {tuple(ray_directions.shape)} differ")
    if not (box_side > 0 and math.isfinite(box_side)):
        raise RuntimeError(f"{who}: box_side must be positive and finite, got {box_side}")
    b, r = ray_origins.shape[:2]
    t_near = torch.empty(b, r, device=ray_origins.device, dtype=torch.float32)
    t_far = torch.empty(b, r, device=ray_origins.device, dtype=torch.float32)
    if b * r:
        L.check(L.lib().hfagp_ray_limits_box(_ptr(ray_origins), _ptr(ray_directions), _ptr(t_near), _ptr(t_far), b * r, float(box_side),
                                             _stream()), who)
    return t_near, t_far


def ray_limits_grid(ray_origins: torch.Tensor, ray_directions: torch.Tensor, occ):
    """(t_near, t_far), each [B,R]: per ray the entry of the FIRST and the exit of the LAST occupied cell of the `OccupancyGrid`
    ``occ`` it passes through at t ≥ 0 (t_near clamped below at 0: an origin inside an occupied cell starts at the origin), for
    `raymarch_rays(..., t_near=, t_far=)`.  A ray that meets no occupied cell, misses the cube, has a zero direction or the box
    kernel's 0 · inf case gets (+inf, −inf): an empty ray to the ray marcher.  Directions of any length, t in units of d.  The
    grid's batch is B or 1 (one grid for every frame).  One launch (hfagp_ray_limits_grid: a 3-D DDA bounded at 3 G + 3 steps, every
    t recomputed from its plane index); `cam_utils.ray_limits_grid` is its brute-force reference in torch."""
    who = "ray_limits_grid"
    for name, t in (("ray_origins", ray_origins), ("ray_directions", ray_directions)):
        if _chk(t, f"{who}: {name}").dim() != 3 or t.shape[2] != 3:
            raise RuntimeError(f"{who}: {name} must be [B, R, 3], got {tuple(t.shape)}")
    if ray_origins.shape != ray_directions.shape:
        raise RuntimeError(f"{who}: ray_origins {tuple(ray_origins.shape)} and ray_directions {tuple(ray_directions.shape)} differ")
    bits = getattr(occ, "bits", None)
    if bits is None:
        raise RuntimeError(f"{who}: occ must be an OccupancyGrid, got {type(occ).__name__}")
    b, r = ray_origins.shape[:2]
    g = int(occ.resolution)
    if not (bits.is_cuda and bits.device == ray_origins.device and bits.dtype == torch.int32 and bits.is_contiguous() and
            tuple(bits.shape[1:]) == (g, g, (g + 31) // 32)):
        raise RuntimeError(f"{who}: occ.bits must be a contiguous int32 tensor [B, {g}, {g}, {(g + 31) // 32}] on {ray_origins.device}, "
                           f"got {bits.dtype} {tuple(bits.shape)} on {bits.device}")
    if bits.shape[0] not in (1, b):
        raise RuntimeError(f"{who}: the grid's batch must be B = {b} or 1, got {bits.shape[0]}")
    t_near = torch.empty(b, r, device=ray_origins.device, dtype=torch.float32)
    t_far = torch.empty(b, r, device=ray_origins.device, dtype=torch.float32)
    if b * r:
        nb, nr = (b, r) if bits.shape[0] == b else (1, b * r)          # one grid for all frames: the list as one frame
        L.check(L.lib().hfagp_ray_limits_grid(_ptr(ray_origins), _ptr(ray_directions), _ptr(bits), _ptr(t_near), _ptr(t_far), nb, nr, g,
                                              float(occ.cube_length), _stream()), who)
    return t_near, t_far


def occupancy_pack(vol: torch.Tensor, resolution: int, oversample: int, level: float, dilate: int) -> torch.Tensor:
    """A density lattice → the bits of an `OccupancyGrid`: vol [B, n, n, n] with n = G·k + 1 points per axis (G = ``resolution``,
    k = ``oversample`` ≥ 1; `density_grid`'s layout, iz fastest) → int32 [B, G, G, ceil(G/32)].  A cell is occupied iff one of the
    (k+1)³ lattice points of its closed extent has !(v < level) — faces are shared with the neighbours, a NaN counts — and the grid
    is then dilated by ``dilate`` cells (0 … 8; Chebyshev distance, clipped at the cube).  One launch (hfagp_occupancy_pack), no
    atomics; `occupancy.occupancy_reference` is the same in torch."""
    who = "occupancy_pack"
    g, k, dilate = int(resolution), int(oversample), int(dilate)
    if not 2 <= g <= 256:
        raise ValueError(f"{who}: resolution must be in [2, 256], got {resolution}")
    if k < 1 or g * k + 1 > 1025:
        raise ValueError(f"{who}: oversample must be >= 1 with G * oversample + 1 <= 1025, got {oversample} at G = {g}")
    if not 0 <= dilate <= 8:
        raise ValueError(f"{who}: dilate must be in [0, 8], got {dilate}")
    if math.isnan(float(level)):
        raise ValueError(f"{who}: level is NaN")
    n = g * k + 1
    if _chk(vol, f"{who}: vol").dim() != 4 or tuple(vol.shape[1:]) != (n, n, n):
        raise RuntimeError(f"{who}: vol must be [B, {n}, {n}, {n}] for G = {g}, oversample = {k}, got {tuple(vol.shape)}")
    bits = torch.empty(vol.shape[0], g, g, (g + 31) // 32, device=vol.device, dtype=torch.int32)
    if vol.shape[0]:
        L.check(L.lib().hfagp_occupancy_pack(_ptr(vol), _ptr(bits), vol.shape[0], g, k, float(level), dilate, _stream()), who)
    return bits


def raymarch_normals(planes: torch.Tensor, state: torch.Tensor, *, cam2world: torch.Tensor, intrinsics: torch.Tensor,
                     u_strat: torch.Tensor, u_imp: torch.Tensor, dec_w0: torch.Tensor, dec_b0: torch.Tensor,
                     dec_w1: torch.Tensor, dec_b1: torch.Tensor, res: int, ray_start: float, ray_end: float, box_warp: float,
                     decoder_lr_mul: float, plane_axes: int, white_back: bool, decoder_precision: str,
                     planes_absmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-ray surface normals [B,R,3] (hfagp_raymarch_normals) of the `raymarch(..., state=state)` call with the same arguments:
    N = Σ_s ω_s n_s over the Sc + Sf depth-sorted samples, n = −g·rsqrt(g·g + 1e-12) with g = ∇ₓσ the WORLD-space gradient of the
    raw decoder density (before softplus(σ − 1)), ω the colour weights of the forward.  ‖N‖ ≤ wsum; not normalised; `white_back`
    does not enter.  The result carries no gradient (its backward is `raymarch_normals_bwd`).  No atomics: two calls return the
    same bits."""
    if state is None:
        raise RuntimeError("raymarch_normals: state must be the `raymarch_state` buffer the forward call filled, got None")
    a = L.RaymarchArgs()
    b, _, _, r, _, _ = _ray_args("raymarch_normals", a, planes, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1, res,
                                 ray_start, ray_end, box_warp, decoder_lr_mul, plane_axes, white_back, decoder_precision, planes_absmax, state)
    normal = torch.empty(b, r, 3, device=planes.device, dtype=torch.float32)
    if b == 0:
        return normal
    L.check(L.lib().hfagp_raymarch_normals(C.byref(a), _ptr(normal), _stream()), "raymarch_normals")
    return normal


def raymarch_normals_bwd(g_normal: torch.Tensor, planes: torch.Tensor, state: torch.Tensor, *, cam2world: torch.Tensor,
                         intrinsics: torch.Tensor, u_strat: torch.Tensor, u_imp: torch.Tensor, dec_w0: torch.Tensor,
                         dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, res: int, ray_start: float, ray_end: float,
                         box_warp: float, decoder_lr_mul: float, plane_axes: int, white_back: bool, decoder_precision: str,
                         planes_absmax: Optional[torch.Tensor] = None, d_planes: Optional[torch.Tensor] = None,
                         decoder_grads: bool = False, dec_out=None):
    """Backward of `raymarch_normals(planes, state, ...)` (hfagp_raymarch_normals_bwd) → ``(d_planes, dec)``.  ``g_normal`` [B,R,3]:
    dL/d normal.  Through the compositing weights (the normals as three colours) and through the normals themselves (the second
    derivative of the tri-plane gather: include/hfagp.h has the formulas); the sample depths carry no gradient.

      * ``d_planes``: a [B,3,H,W,32] tensor the plane gradient is ACCUMULATED into (returned); None = fresh zeros.  A tensor shared
        with `raymarch_bwd` must have been through that call FIRST: on mirrored planes it overwrites plane 2, and this kernel adds
        to all three planes at their true texels.
      * ``decoder_grads`` / ``dec_out``: as `raymarch_bwd` — the four decoder-parameter gradients, accumulated into ``dec_out`` when
        given, else into fresh zeros; ``dec`` is None without them.  The colour rows of the second layer receive nothing.
    A ray whose ``g_normal`` is exactly zero touches nothing.  The other keywords are the forward's; pass its ``planes_absmax``."""
    if state is None:
        raise RuntimeError("raymarch_normals_bwd: state must be the `raymarch_state` buffer the forward call filled, got None")
    a = L.RaymarchArgs()
    b, _, _, r, _, _ = _ray_args("raymarch_normals_bwd", a, planes, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1,
                                 res, ray_start, ray_end, box_warp, decoder_lr_mul, plane_axes, white_back, decoder_precision,
                                 planes_absmax, state)
    if _chk(g_normal, "raymarch_normals_bwd: g_normal").shape != (b, r, 3):
        raise RuntimeError(f"raymarch_normals_bwd: g_normal must be [B, R, 3] = [{b}, {r}, 3], got {tuple(g_normal.shape)}")
    if d_planes is None:
        d_planes = torch.zeros_like(planes)
    elif _chk(d_planes, "raymarch_normals_bwd: d_planes").shape != planes.shape:
        raise RuntimeError(f"raymarch_normals_bwd: d_planes must be shaped like planes {tuple(planes.shape)}, got {tuple(d_planes.shape)}")
    out = types.SimpleNamespace(d_dec_w0=None, d_dec_b0=None, d_dec_w1=None, d_dec_b1=None)      # (the entry takes them one by one)
    dec = _dec_grad_out("raymarch_normals_bwd", out, (dec_w0, dec_b0, dec_w1, dec_b1), decoder_grads, dec_out)
    if b == 0:
        return d_planes, dec
    L.check(L.lib().hfagp_raymarch_normals_bwd(C.byref(a), _ptr(g_normal), _ptr(d_planes), out.d_dec_w0, out.d_dec_b0, out.d_dec_w1,
                                               out.d_dec_b1, _stream()), "raymarch_normals_bwd")
    return d_planes, dec


def raymarch_normals_bwd_camera(g_normal: torch.Tensor, planes: torch.Tensor, state: torch.Tensor, *,
                                ray_grad: Optional[torch.Tensor] = None, reduce: bool = True, cam2world: torch.Tensor,
                                intrinsics: torch.Tensor, u_strat: torch.Tensor, u_imp: torch.Tensor, dec_w0: torch.Tensor,
                                dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, res: int, ray_start: float,
                                ray_end: float, box_warp: float, decoder_lr_mul: float, plane_axes: int, white_back: bool,
                                decoder_precision: str, planes_absmax: Optional[torch.Tensor] = None):
    """The camera gradient of `raymarch_normals(planes, state, ...)` (hfagp_raymarch_normals_bwd_camera) →
    ``(d_cam2world [B,16], d_intrinsics [B,9], ray_grad [B,R,6])``.  ``g_normal`` [B,R,3]: dL/d normal.  The sample depths carry no
    gradient; the positions do, through the compositing weights, the decoder's curvature and the mixed second derivative of the
    bilinear tap weights (include/hfagp.h has the formulas).

      * ``ray_grad``: a [B,R,6] tensor the per-ray records (d origin, d direction) are ADDED to — the one `raymarch_bwd_camera`
        returned, so that one reduction serves the whole loss; None = a fresh tensor that is written.
      * ``reduce``: run the reduction over the final ``ray_grad``; False returns (None, None, ray_grad).
    A ray whose ``g_normal`` is exactly zero adds nothing (writes zeros into a fresh tensor).  No atomics: two calls return the same
    bits.  The other keywords are the forward's; pass its ``planes_absmax``."""
    if state is None:
        raise RuntimeError("raymarch_normals_bwd_camera: state must be the `raymarch_state` buffer the forward call filled, got None")
    a = L.RaymarchArgs()
    b, _, _, r, _, _ = _ray_args("raymarch_normals_bwd_camera", a, planes, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0, dec_w1,
                                 dec_b1, res, ray_start, ray_end, box_warp, decoder_lr_mul, plane_axes, white_back, decoder_precision,
                                 planes_absmax, state)
    if _chk(g_normal, "raymarch_normals_bwd_camera: g_normal").shape != (b, r, 3):
        raise RuntimeError(f"raymarch_normals_bwd_camera: g_normal must be [B, R, 3] = [{b}, {r}, 3], got {tuple(g_normal.shape)}")
    accumulate = ray_grad is not None
    if ray_grad is None:
        ray_grad = torch.empty(b, r, 6, device=planes.device, dtype=torch.float32)
    elif _chk(ray_grad, "raymarch_normals_bwd_camera: ray_grad").shape != (b, r, 6):
        raise RuntimeError(f"raymarch_normals_bwd_camera: ray_grad must be [B, R, 6] = [{b}, {r}, 6], got {tuple(ray_grad.shape)}")
    d_c2w = torch.empty(b, 16, device=planes.device, dtype=torch.float32) if reduce else None
    d_intr = torch.empty(b, 9, device=planes.device, dtype=torch.float32) if reduce else None
    if b == 0:
        return d_c2w, d_intr, ray_grad
    L.check(L.lib().hfagp_raymarch_normals_bwd_camera(C.byref(a), _ptr(g_normal), _ptr(ray_grad), int(accumulate), _ptr(d_c2w),
                                                      _ptr(d_intr), _stream()), "raymarch_normals_bwd_camera")
    return d_c2w, d_intr, ray_grad


def _rays_normals_args(who: str, planes, state, g_normal, ray_origins, ray_directions, u_strat, u_imp, t_near, t_far, scene):
    """The RayListArgs of the three list normals ops (`_ray_list_args`), the limits and (B, R); owns the checks of `state` and
    ``g_normal`` (None for the forward)."""
    if state is None:
        raise RuntimeError(f"{who}: state must be the `raymarch_state` buffer the forward call filled, got None")
    a = L.RayListArgs()
    b, _, _, r, _, _, lim = _ray_list_args(who, a, planes, ray_origins, ray_directions, u_strat, u_imp, state=state, t_near=t_near,
                                           t_far=t_far, **scene)
    if g_normal is not None and _chk(g_normal, f"{who}: g_normal").shape != (b, r, 3):
        raise RuntimeError(f"{who}: g_normal must be [B, R, 3] = [{b}, {r}, 3], got {tuple(g_normal.shape)}")
    return a, C.byref(lim) if lim is not None else None, b, r


def raymarch_rays_normals(planes: torch.Tensor, state: torch.Tensor, *, ray_origins: torch.Tensor, ray_directions: torch.Tensor,
                          u_strat: torch.Tensor, u_imp: torch.Tensor, dec_w0: torch.Tensor, dec_b0: torch.Tensor,
                          dec_w1: torch.Tensor, dec_b1: torch.Tensor, ray_start: float, ray_end: float, box_warp: float,
                          decoder_lr_mul: float, plane_axes: int, white_back: bool, decoder_precision: str,
                          planes_absmax: Optional[torch.Tensor] = None, t_near: Optional[torch.Tensor] = None,
                          t_far: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`raymarch_normals` on a ray list (hfagp_raymarch_rays_normals): per-ray surface normals [B,R,3] of the
    `raymarch_rays(..., state=state)` call with the same arguments — N = Σ_s ω_s n_s at the samples o + t·d, world space, not
    normalised, ‖N‖ ≤ wsum; `white_back` does not enter.  ``state``: `raymarch_rays_state`.  ``t_near`` / ``t_far`` [B,R]: that
    call's per-ray limits; an EMPTY ray (limits not finite, or far ≤ near) has no state and gets exactly (0, 0, 0).  The result
    carries no gradient (its backward is `raymarch_rays_normals_bwd`).  No atomics: two calls return the same bits."""
    who = "raymarch_rays_normals"
    a, lim, b, r = _rays_normals_args(who, planes, state, None, ray_origins, ray_directions, u_strat, u_imp, t_near, t_far, dict(
        dec_w0=dec_w0, dec_b0=dec_b0, dec_w1=dec_w1, dec_b1=dec_b1, ray_start=ray_start, ray_end=ray_end, box_warp=box_warp,
        decoder_lr_mul=decoder_lr_mul, plane_axes=plane_axes, white_back=white_back, decoder_precision=decoder_precision,
        planes_absmax=planes_absmax))
    normal = torch.empty(b, r, 3, device=planes.device, dtype=torch.float32)
    if b * r == 0:
        return normal
    L.check(L.lib().hfagp_raymarch_rays_normals(C.byref(a), lim, _ptr(normal), _stream()), who)
    return normal


def raymarch_rays_normals_bwd(g_normal: torch.Tensor, planes: torch.Tensor, state: torch.Tensor, *, ray_origins: torch.Tensor,
                              ray_directions: torch.Tensor, u_strat: torch.Tensor, u_imp: torch.Tensor, dec_w0: torch.Tensor,
                              dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, ray_start: float, ray_end: float,
                              box_warp: float, decoder_lr_mul: float, plane_axes: int, white_back: bool, decoder_precision: str,
                              planes_absmax: Optional[torch.Tensor] = None, t_near: Optional[torch.Tensor] = None,
                              t_far: Optional[torch.Tensor] = None, d_planes: Optional[torch.Tensor] = None,
                              decoder_grads: bool = False, dec_out=None):
    """Backward of `raymarch_rays_normals(planes, state, ...)` (hfagp_raymarch_rays_normals_bwd) → ``(d_planes, dec)``: what
    `raymarch_normals_bwd` is to `raymarch_normals`, with the same ``d_planes`` / ``decoder_grads`` / ``dec_out`` keywords — both
    ACCUMULATED into, and a ``d_planes`` shared with `raymarch_rays_bwd` must have been through that call FIRST (it overwrites
    plane 2 on mirrored planes).  ``g_normal`` [B,R,3]: dL/d normal.  A ray whose ``g_normal`` is exactly zero touches nothing, and
    neither does an empty ray of ``t_near`` / ``t_far`` (its g_normal is not read); the limits and the sample depths carry no
    gradient.  The other keywords are the forward's; pass its ``planes_absmax``."""
    who = "raymarch_rays_normals_bwd"
    a, lim, b, r = _rays_normals_args(who, planes, state, g_normal, ray_origins, ray_directions, u_strat, u_imp, t_near, t_far, dict(
        dec_w0=dec_w0, dec_b0=dec_b0, dec_w1=dec_w1, dec_b1=dec_b1, ray_start=ray_start, ray_end=ray_end, box_warp=box_warp,
        decoder_lr_mul=decoder_lr_mul, plane_axes=plane_axes, white_back=white_back, decoder_precision=decoder_precision,
        planes_absmax=planes_absmax))
    if d_planes is None:
        d_planes = torch.zeros_like(planes)
    elif _chk(d_planes, f"{who}: d_planes").shape != planes.shape:
        raise RuntimeError(f"{who}: d_planes must be shaped like planes {tuple(planes.shape)}, got {tuple(d_planes.shape)}")
    out = types.SimpleNamespace(d_dec_w0=None, d_dec_b0=None, d_dec_w1=None, d_dec_b1=None)      # (the entry takes them one by one)
    dec = _dec_grad_out(who, out, (dec_w0, dec_b0, dec_w1, dec_b1), decoder_grads, dec_out)
    if b * r == 0:
        return d_planes, dec
    L.check(L.lib().hfagp_raymarch_rays_normals_bwd(C.byref(a), lim, _ptr(g_normal), _ptr(d_planes), out.d_dec_w0, out.d_dec_b0,
                                                    out.d_dec_w1, out.d_dec_b1, _stream()), who)
    return d_planes, dec


def raymarch_rays_normals_bwd_rays(g_normal: torch.Tensor, planes: torch.Tensor, state: torch.Tensor, *, d_origins=None,
                                   d_directions=None, ray_origins: torch.Tensor, ray_directions: torch.Tensor,
                                   u_strat: torch.Tensor, u_imp: torch.Tensor, dec_w0: torch.Tensor, dec_b0: torch.Tensor,
                                   dec_w1: torch.Tensor, dec_b1: torch.Tensor, ray_start: float, ray_end: float, box_warp: float,
                                   decoder_lr_mul: float, plane_axes: int, white_back: bool, decoder_precision: str,
                                   planes_absmax: Optional[torch.Tensor] = None, t_near: Optional[torch.Tensor] = None,
                                   t_far: Optional[torch.Tensor] = None):
    """The rays' gradient of `raymarch_rays_normals(planes, state, ...)` (hfagp_raymarch_rays_normals_bwd_rays) →
    ``(d origins, d directions)``, each [B,R,3]: the per-ray record of `raymarch_normals_bwd_camera`, which for a list is the
    answer (no reduction).  ``g_normal`` [B,R,3]: dL/d normal.

      * ``d_origins`` / ``d_directions`` (both or neither): the [B,R,3] tensors `raymarch_rays_bwd_rays` returned, which the normal
        term is ADDED to (and which are returned); None = fresh tensors that are written.
    A ray whose ``g_normal`` is exactly zero, and an empty ray of ``t_near`` / ``t_far``, add nothing (write zeros into fresh
    tensors).  The derivative holds the limits and the sample depths fixed.  No atomics: two calls return the same bits.  The other
    keywords are the forward's; pass its ``planes_absmax``."""
    who = "raymarch_rays_normals_bwd_rays"
    a, lim, b, r = _rays_normals_args(who, planes, state, g_normal, ray_origins, ray_directions, u_strat, u_imp, t_near, t_far, dict(
        dec_w0=dec_w0, dec_b0=dec_b0, dec_w1=dec_w1, dec_b1=dec_b1, ray_start=ray_start, ray_end=ray_end, box_warp=box_warp,
        decoder_lr_mul=decoder_lr_mul, plane_axes=plane_axes, white_back=white_back, decoder_precision=decoder_precision,
        planes_absmax=planes_absmax))
    if (d_origins is None) != (d_directions is None):
        raise RuntimeError(f"{who}: d_origins and d_directions go together (both or neither)")
    accumulate = d_origins is not None
    if not accumulate:
        d_origins = torch.empty(b, r, 3, device=planes.device, dtype=torch.float32)
        d_directions = torch.empty(b, r, 3, device=planes.device, dtype=torch.float32)
    for name, t in (("d_origins", d_origins), ("d_directions", d_directions)):
        if _chk(t, f"{who}: {name}").shape != (b, r, 3):
            raise RuntimeError(f"{who}: {name} must be [B, R, 3] = [{b}, {r}, 3], got {tuple(t.shape)}")
    if b * r == 0:
        return d_origins, d_directions
    L.check(L.lib().hfagp_raymarch_rays_normals_bwd_rays(C.byref(a), lim, _ptr(g_normal), _ptr(d_origins), _ptr(d_directions),
                                                         int(accumulate), _stream()), who)
    return d_origins, d_directions


def planes_query(planes: torch.Tensor, coords: Optional[torch.Tensor] = None, *, grid=None, dec_w0: torch.Tensor,
                 dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, box_warp: float, plane_axes,
                 decoder_lr_mul: float, decoder_precision: str, planes_absmax: Optional[torch.Tensor] = None,
                 want_rgb: bool = True, out: Optional[torch.Tensor] = None):
    """The decoder at points (hfagp_planes_query): raw density and the 32 decoder features, as
    ``oracle.osg_decoder(P, oracle.sample_from_planes(axes, planes, coords, box_warp), lr_mul)``.  Returns ``(sigma, rgb)``,
    rgb None when ``want_rgb`` is False (the sigma-only kernel skips the colour rows of the decoder's last layer).

    planes [B,3,H,W,32] channels-last.  Points, one of:
      * ``coords`` [Bc,M,3] (Bc = 1 or B; 1 queries the same points for every identity) → sigma [B,M,1], rgb [B,M,32];
      * ``grid=(N, cube_length, x_begin, x_count)`` (or just N: the whole lattice, cube_length = box_warp): EG3D's
        create_samples lattice on the exact integer grid, generated in the kernel → sigma [B,x_count,N,N] indexed
        (ix - x_begin, iy, iz), rgb [B,x_count,N,N,32].  ``out`` (grid, sigma only): a [B,x_count,N,N] tensor to write into,
        contiguous inside each identity (a slab view of a whole [B,N,N,N] volume).
    Decoder arithmetic as `raymarch`: 'f16x3' (bound on |planes| from ``planes_absmax`` or one reduction here) or 'fp32'."""
    b, h, w = _planes_dims("planes_query", planes)
    dev = planes.device
    a = L.PlanesQueryArgs()
    if coords is not None:
        if grid is not None:
            raise ValueError("planes_query: pass coords or grid, not both")
        m = _query_points("planes_query", coords, b)
        if out is not None:
            raise ValueError("planes_query: out= is for grid mode")
        sigma = torch.empty(b, m, 1, device=dev, dtype=torch.float32)
        rgb = torch.empty(b, m, 32, device=dev, dtype=torch.float32) if want_rgb else None
        if b == 0 or m == 0:
            return sigma, rgb
        a.coords, a.Bc, a.M = _ptr(coords), coords.shape[0], m
    else:
        if grid is None:
            raise ValueError("planes_query: pass coords or grid")
        n, cube, x0, xc = (grid, None, 0, None) if isinstance(grid, int) else tuple(grid)
        cube = float(box_warp) if cube is None else float(cube)
        xc = n - x0 if xc is None else xc
        if out is not None:
            if want_rgb:
                raise ValueError("planes_query: out= takes the sigma of a sigma-only query (want_rgb=False)")
            if out.shape != (b, xc, n, n) or out.dtype != torch.float32 or not out.is_cuda or \
                    (b > 0 and out[0].numel() > 0 and not out[0].is_contiguous()):
                raise RuntimeError(f"planes_query: out must be a float32 [B, {xc}, {n}, {n}] tensor contiguous per identity")
            sigma = out
        else:
            sigma = torch.empty(b, xc, n, n, device=dev, dtype=torch.float32)
        rgb = torch.empty(b, xc, n, n, 32, device=dev, dtype=torch.float32) if want_rgb else None
        if b == 0 or xc == 0:
            return sigma, rgb
        a.N, a.x_begin, a.x_count, a.cube_length = n, x0, xc, cube
        a.out_stride = sigma.stride(0)
    _fill_decoder("planes_query", a, planes, (dec_w0, dec_b0, dec_w1, dec_b1), decoder_precision, planes_absmax)
    a.planes, a.sigma, a.rgb = _ptr(planes), _ptr(sigma), _ptr(rgb)
    a.B, a.H, a.W, a.plane_axes = b, h, w, _plane_axes_id(plane_axes)
    a.box_warp, a.decoder_lr_mul = box_warp, decoder_lr_mul
    L.check(L.lib().hfagp_planes_query(C.byref(a), _stream()), "planes_query")
    return sigma, rgb


def planes_query_bwd(planes: torch.Tensor, coords: torch.Tensor, g_sigma: Optional[torch.Tensor], g_rgb: Optional[torch.Tensor], *,
                     dec_w0: torch.Tensor, dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, box_warp: float,
                     plane_axes, decoder_lr_mul: float, decoder_precision: str, planes_absmax: Optional[torch.Tensor] = None,
                     d_planes=None, coords_grad: bool = False, decoder_grads: bool = False, dec_out=None):
    """Backward of `planes_query(planes, coords, ...)` (hfagp_planes_query_bwd; explicit points only) → ``(d_planes, d_coords,
    dec)``.  ``g_sigma`` [B,M,1] or [B,M] and ``g_rgb`` [B,M,32]: the upstream gradients, either may be None.

      * ``d_planes``: a [B,3,H,W,32] tensor the plane gradient is ACCUMULATED into (returned), None = fresh zeros, False = not
        wanted (None is returned).  A tensor shared with `raymarch_bwd` must have been through that call FIRST: on mirrored
        planes it overwrites plane 2, and this kernel adds to all three planes at their true texels.
      * ``coords_grad``: also return d_coords [B,M,3] (one row per identity; for broadcast coords [1,M,3] the gradient of the
        shared points is ``d_coords.sum(0, keepdim=True)``), else None.  Points outside the box get exact zeros.
      * ``decoder_grads`` / ``dec_out``: as `raymarch_bwd` — four decoder-parameter gradients, accumulated into ``dec_out``
        when given, else into fresh zeros; ``dec`` is None without them.
    The other keywords are the forward's; pass the ``planes_absmax`` the forward call got, so that the recomputed decoder is
    the one that ran."""
    b, h, w = _planes_dims("planes_query_bwd", planes)
    dev = planes.device
    if coords is None:
        raise ValueError("planes_query_bwd: explicit coords only (grid mode has no backward)")
    m = _query_points("planes_query_bwd", coords, b)
    if g_sigma is None and g_rgb is None:
        raise ValueError("planes_query_bwd: pass g_sigma, g_rgb or both")
    if g_sigma is not None and (_chk(g_sigma, "g_sigma").numel() != b * m or g_sigma.shape[:2] != (b, m)):
        raise RuntimeError(f"planes_query_bwd: g_sigma must be [B, M, 1] = [{b}, {m}, 1], got {tuple(g_sigma.shape)}")
    if g_rgb is not None and _chk(g_rgb, "g_rgb").shape != (b, m, 32):
        raise RuntimeError(f"planes_query_bwd: g_rgb must be [B, M, 32] = [{b}, {m}, 32], got {tuple(g_rgb.shape)}")
    if d_planes is False:
        d_planes = None
        if not (coords_grad or decoder_grads):
            raise ValueError("planes_query_bwd: nothing to compute (d_planes=False without coords_grad or decoder_grads)")
    elif d_planes is None:
        d_planes = torch.zeros_like(planes)
    elif _chk(d_planes, "d_planes").shape != planes.shape:
        raise RuntimeError(f"planes_query_bwd: d_planes must be shaped like planes {tuple(planes.shape)}, got {tuple(d_planes.shape)}")
    d_coords = torch.empty(b, m, 3, device=dev, dtype=torch.float32) if coords_grad else None     # (every point has one writer)
    a = L.PlanesQueryBwdArgs()
    params = (dec_w0, dec_b0, dec_w1, dec_b1)
    dec = _dec_grad_out("planes_query_bwd", a, params, decoder_grads, dec_out)
    if b == 0 or m == 0:
        return d_planes, d_coords, dec
    _fill_decoder("planes_query_bwd", a, planes, params, decoder_precision, planes_absmax)
    a.planes, a.coords, a.Bc, a.M = _ptr(planes), _ptr(coords), coords.shape[0], m
    a.g_sigma, a.g_rgb = _ptr(g_sigma), _ptr(g_rgb)
    a.d_planes, a.d_coords = _ptr(d_planes), _ptr(d_coords)
    a.B, a.H, a.W, a.plane_axes = b, h, w, _plane_axes_id(plane_axes)
    a.box_warp, a.decoder_lr_mul = box_warp, decoder_lr_mul
    L.check(L.lib().hfagp_planes_query_bwd(C.byref(a), _stream()), "planes_query_bwd")
    return d_planes, d_coords, dec


_QUERY_NORMALS_OUT = ("sigma", "rgb", "grad", "normal")


def planes_query_normals(planes: torch.Tensor, coords: torch.Tensor, *, want=_QUERY_NORMALS_OUT, dec_w0: torch.Tensor,
                         dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, box_warp: float, plane_axes,
                         decoder_lr_mul: float, decoder_precision: str, planes_absmax: Optional[torch.Tensor] = None) -> dict:
    """`planes_query` at explicit points with the density gradient and the unit surface normal (hfagp_planes_query_normals), one
    launch → a dict with the keys of ``want`` (any non-empty subset of 'sigma', 'rgb', 'grad', 'normal'):

      * 'sigma' [B,M,1], 'rgb' [B,M,32]: the bits of `planes_query`;
      * 'grad' [B,M,3]: g = ∂σ/∂x of the raw density in WORLD units (zeros padding, align_corners=False; on an integer pixel
        coordinate the one-sided derivative of the cell the forward's floor() picked);
      * 'normal' [B,M,3]: n = −g·rsqrt(g·g + 1e-12), from dense to empty.
    A point outside every plane gets exact zeros in 'grad' and 'normal'.  No atomics: two calls return the same bits.  The results
    carry no gradient (the backward of 'grad' / 'normal' is `planes_query_normals_bwd`, that of 'sigma' / 'rgb' `planes_query_bwd`).
    ``coords`` [Bc,M,3], Bc = 1 or B; the other keywords are `planes_query`'s."""
    who = "planes_query_normals"
    b, h, w = _planes_dims(who, planes)
    dev = planes.device
    want = tuple(want)
    if not want or any(k not in _QUERY_NORMALS_OUT for k in want):
        raise ValueError(f"{who}: want must be a non-empty subset of {_QUERY_NORMALS_OUT}, got {want}")
    if coords is None:
        raise ValueError(f"{who}: explicit coords only (no grid mode)")
    m = _query_points(who, coords, b)
    width = {"sigma": 1, "rgb": 32, "grad": 3, "normal": 3}
    out = {k: torch.empty(b, m, width[k], device=dev, dtype=torch.float32) for k in _QUERY_NORMALS_OUT if k in want}
    if b == 0 or m == 0:
        return out
    a = L.PlanesQueryArgs()
    a.coords, a.Bc, a.M = _ptr(coords), coords.shape[0], m
    _fill_decoder(who, a, planes, (dec_w0, dec_b0, dec_w1, dec_b1), decoder_precision, planes_absmax)
    a.planes, a.sigma, a.rgb = _ptr(planes), _ptr(out.get("sigma")), _ptr(out.get("rgb"))
    a.B, a.H, a.W, a.plane_axes = b, h, w, _plane_axes_id(plane_axes)
    a.box_warp, a.decoder_lr_mul = box_warp, decoder_lr_mul
    L.check(L.lib().hfagp_planes_query_normals(C.byref(a), _ptr(out.get("grad")), _ptr(out.get("normal")), _stream()), who)
    return out


def planes_query_normals_bwd(planes: torch.Tensor, coords: torch.Tensor, g_grad: Optional[torch.Tensor],
                             g_normal: Optional[torch.Tensor], *, dec_w0: torch.Tensor, dec_b0: torch.Tensor, dec_w1: torch.Tensor,
                             dec_b1: torch.Tensor, box_warp: float, plane_axes, decoder_lr_mul: float, decoder_precision: str,
                             planes_absmax: Optional[torch.Tensor] = None, d_planes=None, decoder_grads: bool = False, dec_out=None):
    """Backward of the 'grad' / 'normal' outputs of `planes_query_normals(planes, coords, ...)` (hfagp_planes_query_normals_bwd) →
    ``(d_planes, dec)``.  ``g_grad`` and ``g_normal`` [B,M,3]: dL/d grad and dL/d normal, either may be None.  The second derivative
    of the tri-plane gather plus decoder (include/hfagp.h has the formulas); the gradients of 'sigma' / 'rgb' are `planes_query_bwd`'s
    — a caller with both runs both into the same buffers.  There is no gradient w.r.t. the points.

      * ``d_planes``: a [B,3,H,W,32] tensor the plane gradient is ACCUMULATED into (returned), None = fresh zeros, False = not
        wanted (None is returned; needs ``decoder_grads``).  A tensor shared with `raymarch_bwd` must have been through that call
        FIRST: on mirrored planes it overwrites plane 2, and this kernel adds to all three planes at their true texels.
      * ``decoder_grads`` / ``dec_out``: as `planes_query_bwd`.  The colour rows of dec_w1 and all of dec_b1 receive nothing.
    A point whose two upstream vectors are exactly zero touches nothing.  The other keywords are the forward's; pass its
    ``planes_absmax``."""
    who = "planes_query_normals_bwd"
    b, h, w = _planes_dims(who, planes)
    if coords is None:
        raise ValueError(f"{who}: explicit coords only (no grid mode)")
    m = _query_points(who, coords, b)
    if g_grad is None and g_normal is None:
        raise ValueError(f"{who}: pass g_grad, g_normal or both")
    for name, t in (("g_grad", g_grad), ("g_normal", g_normal)):
        if t is not None and _chk(t, f"{who}: {name}").shape != (b, m, 3):
            raise RuntimeError(f"{who}: {name} must be [B, M, 3] = [{b}, {m}, 3], got {tuple(t.shape)}")
    if d_planes is False:
        d_planes = None
        if not decoder_grads:
            raise ValueError(f"{who}: nothing to compute (d_planes=False without decoder_grads)")
    elif d_planes is None:
        d_planes = torch.zeros_like(planes)
    elif _chk(d_planes, f"{who}: d_planes").shape != planes.shape:
        raise RuntimeError(f"{who}: d_planes must be shaped like planes {tuple(planes.shape)}, got {tuple(d_planes.shape)}")
    a = L.PlanesQueryBwdArgs()
    params = (dec_w0, dec_b0, dec_w1, dec_b1)
    dec = _dec_grad_out(who, a, params, decoder_grads, dec_out)
    if b == 0 or m == 0:
        return d_planes, dec
    _fill_decoder(who, a, planes, params, decoder_precision, planes_absmax)
    a.planes, a.coords, a.Bc, a.M = _ptr(planes), _ptr(coords), coords.shape[0], m
    a.d_planes = _ptr(d_planes)
    a.B, a.H, a.W, a.plane_axes = b, h, w, _plane_axes_id(plane_axes)
    a.box_warp, a.decoder_lr_mul = box_warp, decoder_lr_mul
    L.check(L.lib().hfagp_planes_query_normals_bwd(C.byref(a), _ptr(g_grad), _ptr(g_normal), _stream()), who)
    return d_planes, dec


_TRACE_OUT = ("hit", "cell", "t", "point", "sigma", "sigma_grad", "normal")


def trace_rays(planes: torch.Tensor, origins: torch.Tensor, directions: torch.Tensor, t_near: torch.Tensor, t_far: torch.Tensor,
               level: float, steps: int = 128, refine: int = 8, planes_absmax: Optional[torch.Tensor] = None, want=_TRACE_OUT, *,
               dec_w0: torch.Tensor, dec_b0: torch.Tensor, dec_w1: torch.Tensor, dec_b1: torch.Tensor, box_warp: float, plane_axes,
               decoder_lr_mul: float, decoder_precision: str) -> dict:
    """The first hit of every ray with the iso-surface σ = ``level`` of the raw density (hfagp_trace_rays), one launch → a dict with
    the keys of ``want`` (any non-empty subset of 'hit', 'cell', 't', 'point', 'sigma', 'sigma_grad', 'normal'):

      * 'hit' [B,R] uint8 and 'cell' [B,R] int32: the first node i of t_i = t_near + i·(t_far − t_near)/steps (t_steps = t_far) with
        σ(o + t_i·d) ≥ level; −1 for a miss; 0 when the origin is inside already;
      * 't' [B,R]: for cell > 0 the root in [t_{cell−1}, t_cell] after ``refine`` bisections and one secant step, t_near for cell 0;
      * 'point' [B,R,3] = o + t·d; 'sigma' [B,R], 'sigma_grad' [B,R,3], 'normal' [B,R,3]: `planes_query_normals` at that point (its bits).
    Rays [B,R,3] with limits [B,R] as `raymarch_rays(t_near=, t_far=)` takes them (directions not normalised); a ray whose limits
    are not both finite with t_far > t_near is empty: a miss.  A miss has exact zeros in every float output.  ``level`` in the unit
    of `planes_query`'s sigma (before any softplus), ``steps`` in [1, 4096], ``refine`` in [0, 30].  No atomics: two calls return
    the same bits, whatever ``want`` is.  Nothing carries a gradient.  The decoder keywords are `planes_query`'s."""
    who = "trace_rays"
    b, h, w = _planes_dims(who, planes)
    dev = planes.device
    want = tuple(want)
    if not want or any(k not in _TRACE_OUT for k in want):
        raise ValueError(f"{who}: want must be a non-empty subset of {_TRACE_OUT}, got {want}")
    if not 1 <= int(steps) <= 4096:
        raise ValueError(f"{who}: steps must be in [1, 4096], got {steps}")
    if not 0 <= int(refine) <= 30:
        raise ValueError(f"{who}: refine must be in [0, 30], got {refine}")
    for name, t in (("origins", origins), ("directions", directions)):
        if _chk(t, f"{who}: {name}").dim() != 3 or t.shape[0] != b or t.shape[2] != 3:
            raise RuntimeError(f"{who}: {name} must be [B={b}, R, 3], got {tuple(t.shape)}")
    if origins.shape != directions.shape:
        raise RuntimeError(f"{who}: origins {tuple(origins.shape)} and directions {tuple(directions.shape)} differ")
    r = origins.shape[1]
    for name, t in (("t_near", t_near), ("t_far", t_far)):
        if _chk(t, f"{who}: {name}").shape != (b, r):
            raise RuntimeError(f"{who}: {name} must be [B, R] = [{b}, {r}], got {tuple(t.shape)}")
    shape = {"hit": ((b, r), torch.uint8), "cell": ((b, r), torch.int32), "t": ((b, r), torch.float32),
             "point": ((b, r, 3), torch.float32), "sigma": ((b, r), torch.float32), "sigma_grad": ((b, r, 3), torch.float32),
             "normal": ((b, r, 3), torch.float32)}
    out = {k: torch.empty(shape[k][0], device=dev, dtype=shape[k][1]) for k in _TRACE_OUT if k in want}
    if b == 0 or r == 0:
        return out
    a = L.TraceRaysArgs()
    _fill_decoder(who, a, planes, (dec_w0, dec_b0, dec_w1, dec_b1), decoder_precision, planes_absmax)
    a.planes, a.ray_origins, a.ray_directions, a.t_near, a.t_far = (_ptr(t) for t in (planes, origins, directions, t_near, t_far))
    for k in _TRACE_OUT:
        setattr(a, k, _ptr(out.get(k)))
    a.R, a.B, a.H, a.W, a.plane_axes = r, b, h, w, _plane_axes_id(plane_axes)
    a.steps, a.refine, a.level = int(steps), int(refine), float(level)
    a.box_warp, a.decoder_lr_mul = box_warp, decoder_lr_mul
    L.check(L.lib().hfagp_trace_rays(C.byref(a), _stream()), who)
    return out


_MESH_OUT = ("hit", "face", "t", "bary", "point", "normal", "front")


def trace_mesh(tri: torch.Tensor, origins: torch.Tensor, directions: torch.Tensor, t_near: torch.Tensor, t_far: torch.Tensor,
               grid=None, want=_MESH_OUT) -> dict:
    """The first hit of every ray with a triangle mesh (hfagp_trace_mesh), one launch → a dict with the keys of ``want`` (any
    non-empty subset of 'hit', 'face', 't', 'bary', 'point', 'normal', 'front'), to the definition of
    `mesh.trace_mesh_reference` in float32: 'hit' and 'front' [B,R] uint8, 'face' [B,R] int32 (−1 for a miss), 't' [B,R], 'bary',
    'point', 'normal' [B,R,3]; a miss has exact zeros in every float output.
    ``tri`` [B or 1, F, 9]: the vertices (a, b, c) of every face (`mesh.TriangleMesh.tri`); rays [B,R,3] with limits [B,R]
    (directions not normalised).  ``grid`` = None: brute force, every ray against every face.  ``grid`` = (cell_start
    [B or 1, G³+1] int32, cell_faces [P] int32, box [B or 1, 6] float32, G) as `mesh.TriangleMesh.build_grid` makes and checks them:
    the rays walk the cells and test the faces of their lists — the same faces win, to the bit, up to the float32 phantom candidates
    of near-degenerate or grazing faces, which only brute force is sure to report.  This launcher checks shapes and
    dtypes only (no synchronisation); the kernel clamps what it reads from the lists, so their content cannot make it read out of
    bounds.  No atomics: two calls return the same bits.  Nothing carries a gradient."""
    who = "trace_mesh"
    want = tuple(want)
    if not want or any(k not in _MESH_OUT for k in want):
        raise ValueError(f"{who}: want must be a non-empty subset of {_MESH_OUT}, got {want}")
    for name, t in (("origins", origins), ("directions", directions)):
        if _chk(t, f"{who}: {name}").dim() != 3 or t.shape[2] != 3:
            raise RuntimeError(f"{who}: {name} must be [B, R, 3], got {tuple(t.shape)}")
    if origins.shape != directions.shape:
        raise RuntimeError(f"{who}: origins {tuple(origins.shape)} and directions {tuple(directions.shape)} differ")
    b, r = origins.shape[:2]
    dev = origins.device
    if _chk(tri, f"{who}: tri").dim() != 3 or tri.shape[2] != 9 or (tri.shape[0] != 1 and tri.shape[0] != b) or tri.device != dev:
        raise RuntimeError(f"{who}: tri must be [B or 1, F, 9] on {dev} for B = {b}, got {tuple(tri.shape)} on {tri.device}")
    frames, f = tri.shape[:2]
    for name, t in (("t_near", t_near), ("t_far", t_far)):
        _chk_operand(who, name, t, (b, r), origins)
    a = L.TraceMeshArgs()
    if grid is not None and f > 0:
        cell_start, cell_faces, box, g = grid
        g = int(g)
        if not 1 <= g <= 256:
            raise ValueError(f"{who}: grid resolution must be in [1, 256], got {g}")
        for name, t, shape in (("cell_start", cell_start, (frames, g ** 3 + 1)), ("cell_faces", cell_faces, tuple(cell_faces.shape[:1]))):
            if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
                raise RuntimeError(f"{who}: grid {name} must be a contiguous int32 tensor {list(shape)} on {dev}, got "
                                   f"{list(t.shape)} {t.dtype} on {t.device}")
        _chk_operand(who, "grid box", box, (frames, 6), origins)
        a.cell_start, a.cell_faces, a.grid_box, a.G, a.n_pairs = _ptr(cell_start), _ptr(cell_faces), _ptr(box), g, cell_faces.shape[0]
    shape = {"hit": ((b, r), torch.uint8), "face": ((b, r), torch.int32), "t": ((b, r), torch.float32),
             "bary": ((b, r, 3), torch.float32), "point": ((b, r, 3), torch.float32), "normal": ((b, r, 3), torch.float32),
             "front": ((b, r), torch.uint8)}
    out = {k: torch.empty(shape[k][0], device=dev, dtype=shape[k][1]) for k in _MESH_OUT if k in want}
    if b == 0 or r == 0:
        return out
    a.tri, a.ray_origins, a.ray_directions, a.t_near, a.t_far = (_ptr(t) for t in (tri, origins, directions, t_near, t_far))
    for k in _MESH_OUT:
        setattr(a, k, _ptr(out.get(k)))
    a.R, a.B, a.F, a.tri_frames = r, b, f, (b if frames == b else 1)
    L.check(L.lib().hfagp_trace_mesh(C.byref(a), _stream()), who)
    return out


def marching_cubes(volume: torch.Tensor, level: float, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Iso-surface ``volume > level`` of a float32 [n0, n1, n2] volume (hfagp_marching_cubes_count / _emit) → ``(verts [V, 3]
    float32, faces [F, 3] int32)`` on the volume's device.  Vertices ``origin + spacing * p`` at the crossed lattice edges,
    welded, in the order of include/hfagp.h (owning point, then axis); faces counter-clockwise seen from outside (normals
    toward decreasing values).  Count, one synchronisation to read the two totals, allocate, emit.  Forward only."""
    _chk(volume, "volume")
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise RuntimeError(f"marching_cubes: volume must be [n0, n1, n2] with every extent >= 2, got {tuple(volume.shape)}")
    if torch.is_grad_enabled() and volume.requires_grad:
        raise RuntimeError("marching_cubes: wrap in `torch.no_grad()`; the extraction has no backward")
    dev = volume.device
    n0, n1, n2 = volume.shape
    h = L.lib()
    ws = torch.empty(h.hfagp_marching_cubes_workspace_bytes(n0, n1, n2) // 8, device=dev, dtype=torch.int64)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    a = L.MarchingCubesArgs()
    a.volume, a.workspace, a.counts, a.workspace_bytes = _ptr(volume), _ptr(ws), _ptr(counts), ws.numel() * 8
    a.n0, a.n1, a.n2, a.level = n0, n1, n2, float(level)
    a.origin[:] = [float(x) for x in origin]
    a.spacing[:] = [float(x) for x in spacing]
    L.check(h.hfagp_marching_cubes_count(C.byref(a), _stream()), "marching_cubes")
    nv, nf = (int(x) for x in counts.cpu())
    verts = torch.empty(nv, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(nf, 3, device=dev, dtype=torch.int32)
    if nv == 0 and nf == 0:
        return verts, faces
    a.verts, a.faces, a.vert_capacity, a.face_capacity = _ptr(verts), _ptr(faces), nv, nf
    L.check(h.hfagp_marching_cubes_emit(C.byref(a), _stream()), "marching_cubes")
    return verts, faces


def depth_clamp_(depth: torch.Tensor, tminmax: torch.Tensor, empty_rays: bool = False) -> torch.Tensor:
    """In place: depth.clamp_(tminmax[..., 0].min(), tminmax[..., 1].max()) — MipRayMarcher2's batch-global depth clamp — as ONE
    launch (hfagp_depth_clamp).  ``empty_rays``: a `raymarch_rays` call with per-ray limits, whose empty rays carry depth +inf and
    (+inf, −inf): they stay out of the range (the min / max ignore them) and get its upper end, as EG3D's zero-opacity ray does; a
    call WITHOUT a valid ray has the range (+inf, −inf), and every depth becomes 0 (no host sync: a `where` on the result)."""
    _chk(depth, "depth")
    _chk(tminmax, "tminmax")
    n = depth.numel()
    L.check(L.lib().hfagp_depth_clamp(_ptr(depth), _ptr(tminmax), n, _stream()), "depth_clamp")
    if empty_rays:          # (after the clamp a depth is non-finite iff an end of the range is)
        depth.copy_(torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth)))
    return depth


def raymarch_state(b: int, res: int, sc: int, sf: int, device) -> torch.Tensor:
    """Buffer for `raymarch(..., state=)` / `raymarch_bwd(..., state=)`: [B, R, 35 (Sc + Sf)] floats = 13.4 KB per ray at 48 + 48."""
    return torch.empty(b, res * res, (sc + sf) * 35, device=device, dtype=torch.float32)


def raymarch_rays_state(b: int, r: int, sc: int, sf: int, device) -> torch.Tensor:
    """`raymarch_state` for a list of ``r`` rays per frame: the buffer of `raymarch_rays(..., state=)` / `raymarch_rays_bwd(..., state=)`."""
    return torch.empty(b, r, (sc + sf) * 35, device=device, dtype=torch.float32)


def _decoder_bound(planes: torch.Tensor, decoder_precision: str, planes_absmax: Optional[torch.Tensor]):
    """The 64-slot bound on |planes| of the 16-bit decoder (None for the exact fp32 decoder)."""
    if decoder_precision == "fp32":
        return None
    if decoder_precision != "f16x3":
        raise ValueError(f"decoder_precision must be 'fp32' or 'f16x3', got {decoder_precision!r}")
    if planes_absmax is None:
        planes_absmax = planes.abs().amax().expand(L.ABSMAX_FLOATS).contiguous()
    return _chk(planes_absmax, "planes_absmax")


# ----------------------------------------------------------------------------- antialiased resample (synthesis at any ray resolution)
AA_KMAX = 9              # HFAGP_RESIZE_AA_KMAX: taps per output, and outputs per input, at ratios within [1/4, 4]
_AA_TABLES = {}          # (n_in, n_out) -> (forward table, transposed table, dense float64 matrix), on the host
_AA_DEVICE = {}          # (n_in, n_out, device) -> (forward table, transposed table) on the device


def _aa_pack(start, count, weights) -> torch.Tensor:
    """One axis table as the kernels read it: int32 [n, 2 + AA_KMAX], a row = start, count, then the fp32 weights' bits."""
    n = len(start)
    t = torch.zeros(n, 2 + AA_KMAX, dtype=torch.int32)
    t[:, 0] = torch.tensor(start, dtype=torch.int32)
    t[:, 1] = torch.tensor(count, dtype=torch.int32)
    t[:, 2:] = weights.view(torch.int32)
    return t


def _aa_unpack(table: torch.Tensor):
    """(start [n], count [n], weights [n, AA_KMAX] fp32) of a table of `_aa_tables`."""
    return table[:, 0], table[:, 1], table[:, 2:].contiguous().view(torch.float32)


def _aa_tables(n_in: int, n_out: int):
    """One axis of torch's antialiased bilinear resize (`_upsample_bilinear2d_aa`, align_corners=False) n_in → n_out, built in
    float64: with s = n_in / n_out, support = max(s, 1), inv = 1 / max(s, 1), output i reads the inputs
    [max(0, int(c − support + 0.5)), min(n_in, int(c + support + 0.5))) around c = s (i + 0.5) with the weights
    max(0, 1 − |(j − c + 0.5) inv|) divided by their sum.
    Returns (forward, transposed, dense) as CPU tensors: `forward` [n_out, 2 + AA_KMAX] int32 — per output its first input, its
    number of taps and the fp32 weights (`_aa_unpack`); `transposed` [n_in, 2 + AA_KMAX] — per input the (consecutive) outputs
    that read it and the same fp32 weights, the adjoint in gather form; `dense` [n_out, n_in] float64, the unrounded matrix.
    ValueError outside n_out / 4 <= n_in <= 4 n_out: within it no output has more than AA_KMAX taps and no input more than
    AA_KMAX readers (asserted)."""
    n_in, n_out = int(n_in), int(n_out)
    hit = _AA_TABLES.get((n_in, n_out))
    if hit is not None:
        return hit
    if n_in < 1 or n_out < 1 or 4 * n_in < n_out or n_in > 4 * n_out:
        raise ValueError(f"resize_aa: {n_in} -> {n_out} is outside the supported ratios n_out / 4 <= n_in <= 4 n_out")
    s = n_in / n_out
    support, inv = max(s, 1.0), 1.0 / max(s, 1.0)
    dense = torch.zeros(n_out, n_in, dtype=torch.float64)
    lo_hi = []
    for i in range(n_out):
        c = s * (i + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        j = torch.arange(lo, hi, dtype=torch.float64)
        w = (1.0 - ((j - c + 0.5) * inv).abs()).clamp_min(0.0)
        dense[i, lo:hi] = w / w.sum()
        lo_hi.append((lo, hi))
    assert max(hi - lo for lo, hi in lo_hi) <= AA_KMAX, (n_in, n_out)
    w32 = dense.float()
    fw = torch.zeros(n_out, AA_KMAX)
    for i, (lo, hi) in enumerate(lo_hi):
        fw[i, :hi - lo] = w32[i, lo:hi]
    forward = _aa_pack([lo for lo, _ in lo_hi], [hi - lo for lo, hi in lo_hi], fw)
    # the windows move monotonically with i: the outputs that read input j are consecutive
    first, count = [], []
    tw = torch.zeros(n_in, AA_KMAX)
    for j in range(n_in):
        readers = [i for i, (lo, hi) in enumerate(lo_hi) if lo <= j < hi]
        assert readers == list(range(readers[0], readers[0] + len(readers))) if readers else True, (n_in, n_out, j)
        assert len(readers) <= AA_KMAX, (n_in, n_out, j)
        first.append(readers[0] if readers else 0)
        count.append(len(readers))
        if readers:
            tw[j, :len(readers)] = w32[readers[0]:readers[0] + len(readers), j]
    hit = _AA_TABLES[(n_in, n_out)] = (forward, _aa_pack(first, count, tw), dense)
    return hit


def _aa_device_tables(n_in: int, n_out: int, device):
    key = (int(n_in), int(n_out), device)
    hit = _AA_DEVICE.get(key)
    if hit is None:
        forward, transposed, _ = _aa_tables(n_in, n_out)
        hit = _AA_DEVICE[key] = (forward.to(device), transposed.to(device))
    return hit


def _resize_aa_args(who: str, src: torch.Tensor, in_hw, out_hw, adjoint: bool):
    """The ResizeAaArgs of both directions and the destination tensor: `src` is x [B,Hi,Wi,C] (forward) or g_y [B,Ho,Wo,C]
    (adjoint, read through the transposed tables).  Owns the checks of `src` and of the ratios (ValueError)."""
    _chk(src, f"{who}: {'g_y' if adjoint else 'x'}")
    (hi, wi), (ho, wo) = (int(v) for v in in_hw), (int(v) for v in out_hw)
    if src.dim() != 4 or tuple(src.shape[1:3]) != ((ho, wo) if adjoint else (hi, wi)) or src.shape[3] % 4:
        raise RuntimeError(f"{who}: expected a channels-last [B, {ho if adjoint else hi}, {wo if adjoint else wi}, C] tensor with "
                           f"C a multiple of 4, got {tuple(src.shape)}")
    b, c = src.shape[0], src.shape[3]
    th, tw = (_aa_device_tables(n_in, n_out, src.device)[int(adjoint)] for n_in, n_out in ((hi, ho), (wi, wo)))
    dst = torch.empty((b, hi, wi, c) if adjoint else (b, ho, wo, c), device=src.device, dtype=torch.float32)
    a = L.ResizeAaArgs()
    a.src, a.dst, a.table_h, a.table_w = _ptr(src), _ptr(dst), _ptr(th), _ptr(tw)
    a.B, a.Hi, a.Wi, a.Ho, a.Wo, a.C, a.kmax = b, hi, wi, ho, wo, c, AA_KMAX
    return a, dst


def resize_aa(x: torch.Tensor, out_hw) -> torch.Tensor:
    """x [B,Hi,Wi,C] channels-last, C % 4 == 0 → [B,Ho,Wo,C]: F.interpolate(mode='bilinear', align_corners=False, antialias=True)
    per channel (EG3D's SuperresolutionHybrid8XDC resize of the feature image and the raw RGB), one launch; the per-axis tap
    tables come from the host (`_aa_tables`, cached per size and device)."""
    a, y = _resize_aa_args("resize_aa", x, x.shape[1:3], out_hw, False)
    if y.numel():
        L.check(L.lib().hfagp_resize_aa_fwd(C.byref(a), _stream()), "resize_aa_fwd")
    return y


def resize_aa_bwd(g_y: torch.Tensor, in_hw, g_nchw3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of `resize_aa`: g_y [B,Ho,Wo,C] → g_x [B,Hi,Wi,C], a gather over the transposed tables — every element written once,
    in a fixed order (two calls give the same bits).  `g_nchw3` [B,3,Hi,Wi] is added to channels 0..2 in the same pass: the gradient
    of 'image_raw', which is those channels of the unresampled feature image."""
    a, g_x = _resize_aa_args("resize_aa_bwd", g_y, in_hw, g_y.shape[1:3], True)
    a.add_nchw3 = _ptr(_chk_operand("resize_aa_bwd", "g_nchw3", g_nchw3, (g_x.shape[0], 3) + tuple(g_x.shape[1:3]), g_y))
    if g_x.numel():
        L.check(L.lib().hfagp_resize_aa_bwd(C.byref(a), _stream()), "resize_aa_bwd")
    return g_x


# ----------------------------------------------------------------------------- standalone ops (NCHW)
def _upfirdn2d_raw(x, f, up, down, padding, gain):
    n, c, h, w = x.shape
    fh, fw = f.shape
    px0, px1, py0, py1 = padding
    ho = (h * up + py0 + py1 - fh) // down + 1
    wo = (w * up + px0 + px1 - fw) // down + 1
    y = torch.empty(n, c, ho, wo, device=x.device, dtype=torch.float32)
    L.check(L.lib().hfagp_upfirdn2d_fwd(_ptr(x), _ptr(f), _ptr(y), n, c, h, w, fh, fw, up, down,
                                        px0, px1, py0, py1, gain, _stream()), "upfirdn2d_fwd")
    return y


class _UpFirDn2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f, up, down, padding, gain):
        ctx.save_for_backward(f)
        ctx.cfg = (x.shape, up, down, tuple(padding), gain)
        return _upfirdn2d_raw(x, f, up, down, padding, gain)

    @staticmethod
    def backward(ctx, dy):
        (f,) = ctx.saved_tensors
        (n, c, h, w), up, down, (px0, px1, py0, py1), gain = ctx.cfg
        dy = _chk(dy.contiguous(), "dy")
        dx = torch.empty(n, c, h, w, device=dy.device, dtype=torch.float32)
        L.check(L.lib().hfagp_upfirdn2d_bwd(_ptr(dy), _ptr(f), _ptr(dx), n, c, h, w, f.shape[0], f.shape[1], up, down,
                                            px0, px1, py0, py1, gain, _stream()), "upfirdn2d_bwd")
        return dx, None, None, None, None, None


def upfirdn2d(x: torch.Tensor, f: torch.Tensor, up: int = 1, down: int = 1,
              padding=(0, 0, 0, 0), gain: float = 1.0) -> torch.Tensor:
    """EG3D upfirdn2d(x, f, up, down, padding=[px0,px1,py0,py1], gain) on NCHW fp32; differentiable w.r.t. x."""
    _chk(x, "x")
    _chk(f, "f")
    if x.requires_grad and torch.is_grad_enabled():
        return _UpFirDn2d.apply(x, f, up, down, tuple(padding), gain)
    return _upfirdn2d_raw(x, f, up, down, padding, gain)


def upsample2d(x: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    return upfirdn2d(x, f, up=2, padding=(2, 1, 2, 1), gain=4.0)


def _bias_act_raw(x, b, dim, act, alpha, gain, clamp):
    y = torch.empty_like(x)
    inner = 1
    for s in x.shape[dim + 1:]:
        inner *= s
    L.check(L.lib().hfagp_bias_act_fwd(_ptr(x), _ptr(b), _ptr(y), x.numel(), x.shape[dim], inner, _ACT[act],
                                       alpha, gain, _clamp(clamp), _stream()), "bias_act_fwd")
    return y


class _BiasAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b, dim, act, alpha, gain, clamp):
        y = _bias_act_raw(x, b, dim, act, alpha, gain, clamp)
        ctx.save_for_backward(y)
        ctx.cfg = (dim, act, alpha, gain, clamp, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dim, act, alpha, gain, clamp, has_b = ctx.cfg
        dy = _chk(dy.contiguous(), "dy")
        dx = torch.empty_like(y)
        L.check(L.lib().hfagp_bias_act_bwd(_ptr(dy), _ptr(y), _ptr(dx), y.numel(), _ACT[act], alpha, gain, _clamp(clamp),
                                           _stream()), "bias_act_bwd")
        db = dx.sum([d for d in range(dx.dim()) if d != dim]) if has_b else None
        return dx, db, None, None, None, None, None


def bias_act_bwd(dy: torch.Tensor, y: torch.Tensor, act: str, alpha: float, gain: float,
                 clamp: Optional[float]) -> torch.Tensor:
    """Gradient of bias_act w.r.t. its pre-activation input from the OUTPUT y (EG3D's bias_act backward): dy * gain *
    lrelu'(y) * [|y| < clamp]; any layout (elementwise)."""
    _chk(dy, "dy"), _chk(y, "y")
    dx = torch.empty_like(y)
    L.check(L.lib().hfagp_bias_act_bwd(_ptr(dy), _ptr(y), _ptr(dx), y.numel(), _ACT[act], alpha, gain,
                                       _clamp(clamp), _stream()), "bias_act_bwd")
    return dx


def bias_act(x: torch.Tensor, b: Optional[torch.Tensor] = None, dim: int = 1, act: str = "linear",
             alpha: float = 0.2, gain: Optional[float] = None, clamp: Optional[float] = None) -> torch.Tensor:
    """EG3D bias_act.bias_act(x, b, dim, act, alpha, gain, clamp); differentiable w.r.t. x and b."""
    _chk(x, "x")
    if gain is None:
        gain = math.sqrt(2.0) if act == "lrelu" else 1.0
    if torch.is_grad_enabled() and (x.requires_grad or (b is not None and b.requires_grad)):
        return _BiasAct.apply(x, b, dim, act, alpha, gain, clamp)
    return _bias_act_raw(x, b, dim, act, alpha, gain, clamp)


class _BlurDown(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        b, h, w, c = x.shape
        ctx.shape = (b, h, w, c)
        y = torch.empty(b, h // 2, w // 2, c, device=x.device, dtype=torch.float32)
        L.check(L.lib().hfagp_blur_down_fwd(_ptr(x), _ptr(y), b, h, w, c, _stream()), "blur_down_fwd")
        return y

    @staticmethod
    def backward(ctx, gy):
        b, h, w, c = ctx.shape
        gy = _chk(gy.contiguous(), "gy")
        gx = torch.empty(b, h, w, c, device=gy.device, dtype=torch.float32)
        L.check(L.lib().hfagp_blur_down_bwd(_ptr(gy), _ptr(gx), b, h, w, c, _stream()), "blur_down_bwd")
        return gx


def blur_down(x: torch.Tensor) -> torch.Tensor:
    """Blur(pad (1,1), FIR [1,3,3,1]) + stride-2 sampling of a channels-last tensor [B,H,W,C] -> [B,H/2,W/2,C]
    (the front of the RGB driver's 1x1 skip conv, encoder3d.py ConvLayer(downsample=True)); differentiable."""
    _chk(x, "x")
    return _BlurDown.apply(x)


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    _chk(x, "x")
    b, c, h, w = x.shape
    y = torch.empty(b, h, w, c, device=x.device, dtype=torch.float32)
    L.check(L.lib().hfagp_nchw_to_nhwc(_ptr(x), _ptr(y), b, c, h, w, _stream()), "nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _chk(x, "x")
    b, h, w, c = x.shape
    y = torch.empty(b, c, h, w, device=x.device, dtype=torch.float32)
    L.check(L.lib().hfagp_nhwc_to_nchw(_ptr(x), _ptr(y), b, c, h, w, _stream()), "nhwc_to_nchw")
    return y


# ----------------------------------------------------------------------------- backward pass
_DEV_PW_CHUNKS = os.environ.get("HFAGP_DEV_PW_CHUNKS")


def pointwise_bwd(x: torch.Tensor, dxs_conv=None, s_conv=None, dxs_rgb=None, s_rgb=None, g_rgb_small=None,
                  w_rgb_small=None, s_small=None, g_direct=None, producer: Optional[dict] = None,
                  param_grads: bool = False, y_rgb_small=None, clamp_rgb_small: Optional[float] = None,
                  g_nchw3_a=None, g_nchw3_b=None, deferred: Optional[list] = None):
    """Fused streaming pass over the saved activation x [B,H,W,C] (see include/hfagp.h).  `producer` =
    dict(dcoef, bias, noise, noise_strength, act, alpha, gain, clamp) of the layer that produced x, or None.
    Returns (g_out [B,H,W,C], sums [B,10,C])."""
    _chk(x, "x")
    b, h, w, c = x.shape
    # blocks per sample: at most 4 pixels per thread (the low-resolution layers are latency-bound otherwise: one block
    # walking 64 pixels of 512 channels took 45 us), at most 256 (the partial sums are reduced by a second kernel)
    npl = max(1, 256 // (c // 4))
    # ... and enough blocks to fill the chip: a workgroup waits out one memory round trip per two pixels of its threads, so what
    # counts is how many are RESIDENT — registers allow 5 / 3 / 4 / 3 per CU for the (small toRGB, parameter gradients) variants
    # (the LDS scratch is sized by the rows a variant reduces since round 5; ten rows for all = 40 KB capped it at 4, and 512
    # blocks in total left two per CU: the 512^2 x 64 launches of the fitting step ran at 1.4 - 2.7 TB/s)
    per_cu = {(False, False): 5, (True, False): 3, (False, True): 4, (True, True): 3}[(g_rgb_small is not None, bool(param_grads))]
    c4 = c // 4
    if g_rgb_small is not None and not param_grads and c4 >= 8 and c4 & (c4 - 1) == 0:
        per_cu = 4                     # (the small-toRGB operands shared by shuffles: 128 registers)
    nchunks = max(1, min(max(256, per_cu * 256 // b), -(-(h * w) // (npl * 4))))
    if _DEV_PW_CHUNKS:                                  # developer sweep (tools/dev/pointwise_sweep.py)
        nchunks = max(1, min(int(_DEV_PW_CHUNKS), h * w))
    a = L.PointwiseBwdArgs()
    g_out = torch.empty_like(x)
    partial = torch.empty(b, nchunks, 10, c, device=x.device, dtype=torch.float32)
    sums = torch.empty(b, 10, c, device=x.device, dtype=torch.float32)
    # `deferred` (a list): the partial sums stay un-reduced and (partial, sums) is appended — `reduce_partials_batch(deferred)`
    # fills every `sums` of the list in one launch (its views may be handed around before that)
    a.x, a.g_out, a.partial, a.sums = _ptr(x), _ptr(g_out), _ptr(partial), (None if deferred is not None else _ptr(sums))
    if deferred is not None:
        deferred.append((partial, sums))
    a.dxs_conv, a.s_conv, a.dxs_rgb, a.s_rgb = _ptr(dxs_conv), _ptr(s_conv), _ptr(dxs_rgb), _ptr(s_rgb)
    a.g_rgb_small, a.w_rgb_small, a.s_small, a.g_direct = _ptr(g_rgb_small), _ptr(w_rgb_small), _ptr(s_small), _ptr(g_direct)
    a.B, a.H, a.W, a.C, a.nchunks = b, h, w, c, nchunks
    a.Co = g_rgb_small.shape[1] if g_rgb_small is not None else 0
    a.y_rgb_small = _ptr(y_rgb_small) if (y_rgb_small is not None and clamp_rgb_small is not None) else None
    a.clamp_rgb_small = _clamp(clamp_rgb_small)
    for t in (g_nchw3_a, g_nchw3_b):
        if t is not None and tuple(t.shape) != (b, 3, h, w):
            raise RuntimeError(f"pointwise_bwd: g_nchw3_* must be [B, 3, H, W] = {(b, 3, h, w)}, got {tuple(t.shape)}")
    a.g_nchw3_a, a.g_nchw3_b = _ptr(g_nchw3_a), _ptr(g_nchw3_b)
    a.clamp = -1.0
    a.param_grads = int(param_grads)
    if producer is not None:
        a.has_producer = 1
        a.dcoef_p, a.bias_p, a.noise_p = _ptr(producer.get("dcoef")), _ptr(producer.get("bias")), _ptr(producer.get("noise"))
        a.noise_strength_p = producer.get("noise_strength", 0.0)
        a.noise_strength_dev = _ptr(producer.get("noise_strength_dev"))     # (0-d device tensor: wins over the host value)
        a.act_p = _ACT[producer.get("act", "lrelu")]
        a.alpha, a.gain = producer.get("alpha", 0.2), producer.get("gain", math.sqrt(2.0))
        clamp = producer.get("clamp")
        a.clamp = _clamp(clamp)
    L.check(L.lib().hfagp_pointwise_bwd(C.byref(a), _stream()), "pointwise_bwd")
    return g_out, sums


def upfir_bwd(g_y: torch.Tensor) -> torch.Tensor:
    """g_y [B,2H,2W,C] → parity images of the y_t gradient [2,2,B,H+1,W+1,C]."""
    _chk(g_y, "g_y")
    b, ho, wo, c = g_y.shape
    h, w = ho // 2, wo // 2
    gph = torch.empty(2, 2, b, h + 1, w + 1, c, device=g_y.device, dtype=torch.float32)
    L.check(L.lib().hfagp_upfir_bwd(_ptr(g_y), _ptr(gph), b, h, w, c, _stream()), "upfir_bwd")
    return gph


def upsample2d_bwd(g: torch.Tensor, channels_last: bool) -> torch.Tensor:
    """Adjoint of upsample2d: [B,2H,2W,C] → [B,H,W,C] (channels_last) or [B,C,2H,2W] → [B,C,H,W]."""
    _chk(g, "g")
    if channels_last:
        b, ho, wo, c = g.shape
        out = torch.empty(b, ho // 2, wo // 2, c, device=g.device, dtype=torch.float32)
        outer, inner = b, c
    else:
        b, c, ho, wo = g.shape
        out = torch.empty(b, c, ho // 2, wo // 2, device=g.device, dtype=torch.float32)
        outer, inner = b * c, 1
    L.check(L.lib().hfagp_upsample2d_bwd(_ptr(g), _ptr(out), outer, ho // 2, wo // 2, inner, _stream()), "upsample2d_bwd")
    return out


def planes_to_nhwc(pm: torch.Tensor) -> torch.Tensor:
    _chk(pm, "planes")
    b, three, h, w, cp = pm.shape
    y = torch.empty(b, h, w, 3 * cp, device=pm.device, dtype=torch.float32)
    L.check(L.lib().hfagp_planes_to_nhwc(_ptr(pm), _ptr(y), b, h, w, cp, _stream()), "planes_to_nhwc")
    return y


def planes_sum_to_nhwc(pm: torch.Tensor) -> torch.Tensor:
    """pm [B,V,3,H,W,Cp], the plane gradients of the V frames of every identity → [B,H,W,3Cp]: `planes_to_nhwc` of the sum over the
    views, in one pass (hfagp_planes_sum_to_nhwc: fp32, views added in the order 0 … V−1, no atomics; V = 1 is `planes_to_nhwc`)."""
    _chk(pm, "planes")
    if pm.dim() != 6 or pm.shape[2] != 3:
        raise RuntimeError(f"planes_sum_to_nhwc: pm must be [B, V, 3, H, W, Cp], got {tuple(pm.shape)}")
    b, v, _, h, w, cp = pm.shape
    y = torch.empty(b, h, w, 3 * cp, device=pm.device, dtype=torch.float32)
    L.check(L.lib().hfagp_planes_sum_to_nhwc(_ptr(pm), _ptr(y), b, v, h, w, cp, _stream()), "planes_sum_to_nhwc")
    return y


def style_bwd(ds: torch.Tensor, dd: Optional[torch.Tensor], styles: torch.Tensor, dcoef: Optional[torch.Tensor],
              wsq: Optional[torch.Tensor], affine_w: torch.Tensor, dw: torch.Tensor, style_gain: float = 1.0,
              accumulate: bool = True) -> torch.Tensor:
    """Accumulate d ws for one layer into the row view dw [B, w_dim] (strided view of d_ws); returns
    dstot [B, Cin] = gradient w.r.t. the raw affine output (input of affine_grad)."""
    b, cin = styles.shape
    a = L.StyleBwdArgs()
    dstot = torch.empty(b, cin, device=styles.device, dtype=torch.float32)
    if not ds.is_contiguous():
        ds = ds.contiguous()
    if dd is not None and not dd.is_contiguous():
        dd = dd.contiguous()
    a.ds, a.dd, a.styles, a.dcoef, a.wsq = _ptr(ds), _ptr(dd), _ptr(styles), _ptr(dcoef), _ptr(wsq)
    a.affine_w, a.dstot, a.dw = _ptr(affine_w), _ptr(dstot), dw.data_ptr()
    a.B, a.Cin, a.Cout = b, cin, (dd.shape[1] if dd is not None else 0)
    a.w_dim, a.dw_stride, a.accumulate = affine_w.shape[1], dw.stride(0), int(accumulate)
    a.style_gain = style_gain
    L.check(L.lib().hfagp_style_bwd(C.byref(a), _stream()), "style_bwd")
    return dstot


def style_bwd_batch(items, d_ws: torch.Tensor):
    """All style gradients of a backward pass in two launches.  ``items``: list of (ds [B,Cin] view, dd [B,Cout] view |
    None, styles, dcoef | None, wsq | None, affine_w, row, style_gain); ds / dd may be strided row views (unit inner
    stride) of the reduction tensors.  Accumulates into d_ws[:, row]; returns the dstot [B, Cin] of every item, in the
    order given."""
    order = sorted(range(len(items)), key=lambda i: items[i][6])          # by ws row = by dw pointer
    out = [None] * len(items)
    for c0 in range(0, len(order), 32):
        chunk = order[c0:c0 + 32]
        # a ws row must not straddle two launches (its accumulation is one block's job): cut the chunk at a row boundary
        while c0 + len(chunk) < len(order) and len(chunk) > 1 and items[chunk[-1]][6] == items[order[c0 + len(chunk)]][6]:
            chunk = chunk[:-1]
        if len(chunk) != len(order[c0:c0 + 32]):
            return _style_bwd_each(items, d_ws)                            # (never with <= 32 layers: ffhq has 26)
        arr = (L.StyleBwdItem * len(chunk))()
        for j, i in enumerate(chunk):
            ds, dd, styles, dcoef, wsq, affine_w, row, gain = items[i]
            if ds.stride(-1) != 1 or (dd is not None and dd.stride(-1) != 1):
                raise RuntimeError("style_bwd_batch: ds / dd need unit inner stride")
            b, cin = styles.shape
            dstot = torch.empty(b, cin, device=styles.device, dtype=torch.float32)
            a = arr[j]
            a.ds, a.dd, a.styles, a.dcoef, a.wsq = ds.data_ptr(), (dd.data_ptr() if dd is not None else None), _ptr(styles), \
                _ptr(dcoef), _ptr(wsq)
            a.affine_w, a.dstot = _ptr(affine_w), _ptr(dstot)
            a.dw = d_ws.data_ptr() + row * d_ws.stride(1) * 4
            a.B, a.Cin, a.Cout = b, cin, (dd.shape[1] if dd is not None else 0)
            a.w_dim, a.dw_stride = affine_w.shape[1], d_ws.stride(0)
            a.ds_stride, a.dd_stride = ds.stride(0), (dd.stride(0) if dd is not None else 0)
            a.style_gain = gain
            out[i] = dstot
        L.check(L.lib().hfagp_style_batch_bwd(arr, len(chunk), _stream()), "style_batch_bwd")
    return out


def _style_bwd_each(items, d_ws):
    return [style_bwd(ds, dd, styles, dcoef, wsq, affine_w, d_ws[:, row], gain, accumulate=True)
            for ds, dd, styles, dcoef, wsq, affine_w, row, gain in items]


def conv_wgrad(x: torch.Tensor, styles: Optional[torch.Tensor], g: torch.Tensor, weight: torch.Tensor, mode: int,
               dd: Optional[torch.Tensor] = None, dcoef: Optional[torch.Tensor] = None,
               precision: str = "fp32", ksplit: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient of a modulated conv (see include/hfagp.h): returns dweight like `weight`.  precision 'bf16x3':
    the 3x3 and up-sampling modes with Cin, Cout multiples of 64 run on the split-bf16 MFMA kernel (the 1x1 mode and
    other shapes stay fp32).  `out`: ACCUMULATE into this tensor (the parameter's .grad slice of the trainer's flat buffer)
    instead of returning a new one."""
    _chk(x, "x")
    _chk(g, "g")
    b, h, w, cin = x.shape
    cout = weight.shape[0]
    a = L.WgradArgs()
    if out is not None:
        if out.shape != weight.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise RuntimeError("conv_wgrad: `out` must be a contiguous fp32 tensor of the weight's shape")
        if out.data_ptr() % 16 != 0:
            # (the reducers read and write dW with 16-byte accesses; FlatGrads aligns every slice, a caller's own view
            # may not be)
            raise RuntimeError("conv_wgrad: `out` must be 16-byte aligned (trainer.FlatGrads slices are)")
        a.accumulate = 1
    dweight = torch.empty_like(weight) if out is None else out
    a.x, a.styles, a.g = _ptr(x), _ptr(styles), _ptr(g)
    a.weight, a.dd, a.dcoef, a.dweight = _ptr(_chk(weight.detach(), "weight")), _ptr(dd), _ptr(dcoef), _ptr(dweight)
    if dd is not None:                  # a row view [B, Cout] of pointwise_bwd's sums is read in place (ABI 12 `dd_stride`)
        if dd.dim() != 2 or dd.shape[1] != cout or dd.stride(1) != 1 or dd.dtype != torch.float32:
            raise RuntimeError("conv_wgrad: dd must be [B, Cout] fp32 with unit column stride")
        a.dd_stride = dd.stride(0)
    a.B, a.H, a.W, a.Cin, a.Cout, a.mode = b, h, w, cin, cout, mode
    a.precision = PREC_BF16X3 if precision == "bf16x3" else PREC_F32
    a.ksplit = L.lib().hfagp_wgrad_ksplit(C.byref(a)) if ksplit is None else ksplit      # (the library's split-K policy)
    ws = torch.empty(L.lib().hfagp_wgrad_workspace_bytes(C.byref(a)) // 4, device=x.device, dtype=torch.float32)
    a.workspace = _ptr(ws)
    L.check(L.lib().hfagp_conv_wgrad(C.byref(a), _stream()), "conv_wgrad")
    return dweight


def affine_grad(dstot: torch.Tensor, w: torch.Tensor, dA: torch.Tensor, db: torch.Tensor) -> None:
    """dA [Cin, w_dim] += dstot^T . w / sqrt(w_dim); db [Cin] += sum_b dstot.  w is a row view [B, w_dim] of ws."""
    b, cin = dstot.shape
    L.check(L.lib().hfagp_affine_grad(_ptr(dstot), w.data_ptr(), _ptr(dA), _ptr(db), b, cin, w.shape[1], w.stride(0),
                                      _stream()), "affine_grad")


def reduce_partials_batch(items) -> None:
    """items: (partial [B,nchunks,10,C], sums [B,10,C]) pairs of `pointwise_bwd(..., deferred=list)` calls: one launch per 32."""
    for i0 in range(0, len(items), 32):
        chunk = items[i0:i0 + 32]
        arr = (L.ReducePartialsItem * len(chunk))()
        for a, (partial, sums) in zip(arr, chunk):
            a.partial, a.sums = _ptr(_chk(partial, "partial")), _ptr(_chk(sums, "sums"))
            a.B, a.nchunks, a.n = partial.shape[0], partial.shape[1], partial.shape[2] * partial.shape[3]
        L.check(L.lib().hfagp_reduce_partials_batch(arr, len(chunk), _stream()), "reduce_partials_batch")
    items.clear()


def affine_grad_batch(items) -> None:
    """items: (dstot [B,Cin], w row view [B,w_dim] of ws, dA [Cin,w_dim], db [Cin]) per affine layer; dA / db are accumulated
    into (the parameters' .grad slices): every affine layer of a backward pass in one launch per 32."""
    for i0 in range(0, len(items), 32):
        chunk = items[i0:i0 + 32]
        arr = (L.AffineGradItem * len(chunk))()
        for a, (dstot, w, dA, db) in zip(arr, chunk):
            a.dstot, a.w, a.dA, a.db = _ptr(_chk(dstot, "dstot")), w.data_ptr(), _ptr(_chk(dA, "dA")), _ptr(_chk(db, "db"))
            a.B, a.Cin, a.w_dim, a.w_stride = dstot.shape[0], dstot.shape[1], w.shape[1], w.stride(0)
        L.check(L.lib().hfagp_affine_grad_batch(arr, len(chunk), _stream()), "affine_grad_batch")


def bias_noise_grads(items) -> None:
    """items: (sums [B,10,C] of pointwise_bwd(param_grads=True), dbias [C] or None, dnoise [1] or None): accumulated into."""
    for i0 in range(0, len(items), 32):
        chunk = items[i0:i0 + 32]
        arr = (L.BiasNoiseGradItem * len(chunk))()
        for a, (sums, dbias, dnoise) in zip(arr, chunk):
            a.sums, a.dbias, a.dnoise = _ptr(_chk(sums, "sums")), _ptr(dbias), _ptr(dnoise)
            a.B, a.C = sums.shape[0], sums.shape[2]
        L.check(L.lib().hfagp_bias_noise_grads(arr, len(chunk), _stream()), "bias_noise_grads")


def channel_sum(g: torch.Tensor, out: torch.Tensor, accumulate: bool = True) -> None:
    """out[c] (+)= sum over all leading dims of the channels-last tensor g [..., C]."""
    _chk(g, "g")
    c = g.shape[-1]
    npix = g.numel() // c
    # the kernel walks the tensor as a flat array with a grid stride that is a multiple of C (a thread keeps one channel):
    # nblocks = a multiple of C / gcd(C, 256), about one block per 4096 floats, at most ~1024
    unit = c // math.gcd(c, 256)
    nblocks = unit * int(max(1, min(1024 // unit, g.numel() // (4096 * unit))))
    partial = torch.empty(nblocks, c, device=g.device, dtype=torch.float32)
    L.check(L.lib().hfagp_channel_sum(_ptr(g), _ptr(partial), _ptr(out), npix, c, nblocks, int(accumulate), _stream()),
            "channel_sum")


ROWS_STATS = {"bytes": 0, "chunks": 0, "path": None}      # of the last raymarch_bwd call (bench.py reports it)
_WARNED = set()


def _warn_once(key: str, msg: str) -> None:
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def rows_scratch_cap(device=None) -> int:
    """Bytes the sort + gather ray-march backward may take for its scratch in ONE call: HFAGP_RAYBWD_SCRATCH_GIB (default 16), and
    never more than half of what the device has free right now (plus what torch's allocator already caches)."""
    cap = int(float(os.environ.get("HFAGP_RAYBWD_SCRATCH_GIB", "16")) * (1 << 30))
    try:
        free, _ = torch.cuda.mem_get_info(device)
        free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        cap = min(cap, max(free // 2, 1 << 28))
    except Exception:  # noqa: BLE001 — no device query: the configured cap alone
        pass
    return cap


def depth_range(tminmax: torch.Tensor, empty_rays: bool = False) -> torch.Tensor:
    """tminmax [..., 2] as `raymarch` writes it → [2] device tensor (lo, hi): the batch-global range `depth_clamp_` clamps the
    expected depth to, for `raymarch_bwd(g_depth=..., depth_range=...)`.  No host sync.  ``empty_rays`` (a `raymarch_rays` call with
    per-ray limits): the range is over the valid rays — the (+inf, −inf) of an empty ray does not enter a min / max — and an end
    that is not finite (no valid ray at all) becomes 0, as in `depth_clamp_(..., empty_rays=True)`."""
    _chk(tminmax, "tminmax")
    t = tminmax.reshape(-1, 2)
    rng = torch.stack((t[:, 0].amin(), t[:, 1].amax()))
    return torch.where(torch.isfinite(rng), rng, torch.zeros_like(rng)) if empty_rays else rng


def _check_upstream(who: str, b: int, r: int, g_feat, g_depth, g_wsum, depth_range) -> None:
    """The upstream gradients of `raymarch_bwd` / `raymarch_rays_bwd`: each None or a checked tensor of its shape."""
    if g_feat is not None and _chk(g_feat, f"{who}: g_feat").shape != (b, r, 32):
        raise RuntimeError(f"{who}: g_feat must be [B, R, 32] = [{b}, {r}, 32], got {tuple(g_feat.shape)}")
    for t, name in ((g_depth, "g_depth"), (g_wsum, "g_wsum")):
        if t is not None and _chk(t, f"{who}: {name}").shape != (b, r):
            raise RuntimeError(f"{who}: {name} must be [B, R] = [{b}, {r}], got {tuple(t.shape)}")
    if depth_range is not None and _chk(depth_range, f"{who}: depth_range").shape != (2,):
        raise RuntimeError(f"{who}: depth_range must be [2] (ops.depth_range), got {tuple(depth_range.shape)}")


def _geom_grads(g_depth, g_wsum, depth_range):
    """The RaymarchGeomGrads of a backward call, or None when it has neither a depth nor an opacity gradient."""
    if g_depth is None and g_wsum is None and depth_range is None:
        return None
    gg = L.RaymarchGeomGrads()
    gg.g_depth, gg.g_wsum, gg.depth_range = _ptr(g_depth), _ptr(g_wsum), _ptr(depth_range)
    return gg


def _rows_scratch(who: str, a, need: int, device, divisible: bool, what: str):
    """The scratch plan of pass 2 as sort + gather for the RaymarchBwdArgs ``a``, whose call needs ``need`` bytes (0: the sort does
    not take ``what``) → (cap, None) when the call needs more than `rows_scratch_cap()` allows and is ``divisible``: the caller runs
    it in chunks and reports them to ROWS_STATS; else (None, scratch) — the allocation, set in ``a`` and to be held until the
    launch, or None where the scatter kernels run, which is said once.  The free-memory query is a driver call: only calls that
    could matter pay it (a fitting step's 1.8 GB does not)."""
    cap = rows_scratch_cap(device) if need > (4 << 30) or "HFAGP_RAYBWD_SCRATCH_GIB" in os.environ else (16 << 30)
    if need > cap and divisible:
        return cap, None
    scratch = None
    if need > 0:
        try:
            scratch = torch.empty(need, device=device, dtype=torch.uint8)
            a.rows_scratch, a.rows_scratch_bytes = _ptr(scratch), need
            ROWS_STATS.update(bytes=need, chunks=1, path="rows")
        except torch.cuda.OutOfMemoryError:
            _warn_once("rows_oom", f"{who}: {need / 2**30:.2f} GiB of sort scratch could not be allocated: this call runs the "
                                   f"(~2 x slower) scatter kernels")
    else:
        _warn_once("rows_unsupported", f"{who}: the sort + gather backward does not take {what} (more than 8192 bins per frame): the "
                                       f"(~2 x slower) scatter kernels run")
    if scratch is None:
        ROWS_STATS.update(bytes=0, chunks=1, path="scatter")
    return None, scratch


def raymarch_bwd(g_feat: Optional[torch.Tensor], planes: torch.Tensor, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0,
                 dec_w1, dec_b1, res: int, ray_start: float, ray_end: float, box_warp: float,
                 decoder_lr_mul: float = 1.0, plane_axes: int = 0, white_back: bool = False,
                 return_rec: bool = False, decoder_grads: bool = False, decoder_precision: str = "f16x3",
                 planes_absmax: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                 two_kernel: bool = False, rows: Optional[bool] = None, dec_out=None, _out=None,
                 g_depth: Optional[torch.Tensor] = None, g_wsum: Optional[torch.Tensor] = None,
                 depth_range: Optional[torch.Tensor] = None, rec_out: Optional[list] = None):
    """g_feat [B,R,32] → d planes [B,3,H,W,32].  ``g_depth`` / ``g_wsum`` [B,R]: gradients w.r.t. the CLAMPED expected depth and
    the opacity `raymarch` returns, added to the compositing adjoint (hfagp.h HfagpRaymarchGeomGrads); ``depth_range``
    (`ops.depth_range(tminmax)`, required with g_depth) is the forward's batch-global clamp range; g_feat may be None when one of
    the two is given.  ``state``: what the forward call of this step left behind
    (`raymarch(..., state=)`): the compositing adjoint reads it instead of recomputing.  ``rows``: pass 2 as sort + gather
    (hfagp.h `rows_scratch`, csrc/raymarch_rows.hip) — None = whenever it applies (HFAGP_RAYBWD_ROWS=0 turns the default off: A/B
    timing), False = the scatter kernels.  The sort's scratch (~0.9 GB per frame at 128^2 rays x 96 samples) is bounded by
    `rows_scratch_cap()`: a batch that needs more is processed in frame chunks (round 6; rounds 5 fell back to the 2 x slower scatter
    kernels above 16 GiB, i.e. from B = 19 on, without a word); where the sort does not apply at all (more than 8192 bins per frame)
    or its scratch cannot be allocated, the scatter kernels run and say so once.  ``rec_out``: a list that receives pass 1's
    per-sample records [B,R,Sc+Sf,4] whatever the return form is (`raymarch_bwd_camera` reads them)."""
    who = "raymarch_bwd"
    b, _, _ = _planes_dims(who, planes)
    r = res * res
    _check_upstream(who, b, r, g_feat, g_depth, g_wsum, depth_range)
    d_planes, rec = _out if _out is not None else (
        torch.zeros_like(planes), torch.empty(b, r, u_strat.shape[-1] + u_imp.shape[-1], 4, device=planes.device, dtype=torch.float32))
    if rec_out is not None:
        rec_out.append(rec)
    if rows is None:
        rows = os.environ.get("HFAGP_RAYBWD_ROWS", "1") != "0" and not two_kernel
    dec = _raymarch_bwd_frames(
        g_feat=g_feat, planes=planes, cam2world=cam2world, intrinsics=intrinsics, u_strat=u_strat, u_imp=u_imp, state=state,
        g_depth=g_depth, g_wsum=g_wsum, depth_range=depth_range, d_planes=d_planes, rec=rec, decoder_grads=decoder_grads, dec_out=dec_out,
        rows=rows, two_kernel=two_kernel, dec_w0=dec_w0, dec_b0=dec_b0, dec_w1=dec_w1, dec_b1=dec_b1, res=res, ray_start=ray_start,
        ray_end=ray_end, box_warp=box_warp, decoder_lr_mul=decoder_lr_mul, plane_axes=plane_axes, white_back=white_back,
        decoder_precision=decoder_precision,
        planes_absmax=_decoder_bound(planes, decoder_precision, planes_absmax))       # (one bound for every chunk of the batch)
    if decoder_grads:
        return d_planes, dec
    return (d_planes, rec) if return_rec else d_planes


def _raymarch_bwd_frames(*, g_feat, planes, cam2world, intrinsics, u_strat, u_imp, state, g_depth, g_wsum, depth_range, d_planes, rec,
                         decoder_grads, dec_out, rows, two_kernel, **scene):
    """`raymarch_bwd` of the frames it is given: the whole batch, or — from itself — one chunk of it, which so goes through the same
    scratch decision again (free memory may have shrunk meanwhile).  Fills ``d_planes`` and ``rec`` in place and returns the
    decoder-gradient tuple (None without ``decoder_grads``).  ``scene``: the decoder parameters and the scalars of `_ray_args`."""
    a = L.RaymarchBwdArgs()
    f = a.fwd
    b, h, w, r, sc, sf = _ray_args("raymarch_bwd", f, planes, cam2world, intrinsics, u_strat, u_imp, state=state, **scene)
    dec = _dec_grad_out("raymarch_bwd", a, [scene[k] for k in _DEC], decoder_grads, dec_out)
    a.g_feat, a.d_planes, a.rec = _ptr(g_feat), _ptr(d_planes), _ptr(rec)
    scratch = None
    if rows:
        need = int(L.lib().hfagp_raymarch_bwd_rows_bytes(C.byref(f)))
        cap, scratch = _rows_scratch("raymarch_bwd", a, need, planes.device, b > 1, f"{h} x {w} planes at {f.res}^2 rays")
        if cap is not None:
            # frame chunks: every per-frame input / output is a contiguous slice of the batch; the decoder gradients accumulate
            # in the one `dec`; u_imp is [B * R, Sf]; the depth range is batch-global
            nb = max(1, min(b - 1, int(b * cap // need)))
            per_frame = dict(g_feat=g_feat, planes=planes, cam2world=cam2world, intrinsics=intrinsics, u_strat=u_strat, state=state,
                             g_depth=g_depth, g_wsum=g_wsum, d_planes=d_planes, rec=rec)
            for b0 in range(0, b, nb):
                b1 = min(b, b0 + nb)
                _raymarch_bwd_frames(**{k: None if t is None else t[b0:b1] for k, t in per_frame.items()}, u_imp=u_imp[b0 * r:b1 * r],
                                     depth_range=depth_range, decoder_grads=decoder_grads, dec_out=dec, rows=rows, two_kernel=two_kernel,
                                     **scene)
            ROWS_STATS.update(bytes=min(need, cap), chunks=-(-b // nb), path="rows")
            return dec
    # pass 2 as two kernels (dL/dF through a scratch buffer, then the scatter alone: hfagp.h `df_scratch`) where the column
    # variant applies; 201 MB per frame at 128^2 rays x 96 samples.  OFF by default: measured SLOWER than the fused kernel
    # (B = 2: dL/dF 0.51 ms + scatter 1.41 ms against 1.58 ms fused — the scatter alone is the bound, the arithmetic already
    # hides under it; profiles/r04_raybwd_split.txt).  Kept as the vehicle for work on the scatter.
    if scratch is None and two_kernel and f.plane_axes == 0 and h == w and h <= 256 and b * r * (sc + sf) * 128 <= (4 << 30):
        df = torch.empty(b, r, sc + sf, 32, device=planes.device, dtype=torch.float32)
        a.df_scratch = _ptr(df)
    gg = _geom_grads(g_depth, g_wsum, depth_range)
    if gg is None:
        L.check(L.lib().hfagp_raymarch_bwd(C.byref(a), _stream()), "raymarch_bwd")
    else:
        L.check(L.lib().hfagp_raymarch_bwd_geom(C.byref(a), C.byref(gg), _stream()), "raymarch_bwd")
    return dec


def raymarch_bwd_camera(g_feat: Optional[torch.Tensor], planes: torch.Tensor, rec: torch.Tensor, cam2world, intrinsics, u_strat,
                        u_imp, dec_w0, dec_b0, dec_w1, dec_b1, res: int, ray_start: float, ray_end: float, box_warp: float,
                        decoder_lr_mul: float = 1.0, plane_axes: int = 0, white_back: bool = False,
                        decoder_precision: str = "f16x3", planes_absmax: Optional[torch.Tensor] = None, reduce: bool = True):
    """The camera gradient of the renderer (hfagp_raymarch_bwd_camera) → (d cam2world [B,16], d intrinsics [B,9], ray_grad [B,R,6]:
    d origin, d direction per ray).  ``g_feat`` and the other arguments as in the `raymarch_bwd` call that wrote ``rec`` (its
    ``rec_out=`` / ``return_rec=True``): the depth, opacity and white_back terms are already in the records.  Independent of which
    pass-2 form that call ran; no atomics, two calls return the same bits.  ``reduce=False``: the per-ray records alone, (None, None,
    ray_grad) — for `raymarch_normals_bwd_camera(..., ray_grad=ray_grad)`, whose reduction then serves both."""
    a = L.RaymarchBwdArgs()
    b, _, _, r, sc, sf = _ray_args("raymarch_bwd_camera", a.fwd, planes, cam2world, intrinsics, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1,
                                   res, ray_start, ray_end, box_warp, decoder_lr_mul, plane_axes, white_back, decoder_precision, planes_absmax,
                                   None)
    dev = planes.device
    if _chk(rec, "raymarch_bwd_camera: rec").shape != (b, r, sc + sf, 4):
        raise RuntimeError(f"raymarch_bwd_camera: rec must be [B, R, Sc + Sf, 4] = [{b}, {r}, {sc + sf}, 4], got {tuple(rec.shape)}")
    if g_feat is not None and _chk(g_feat, "raymarch_bwd_camera: g_feat").shape != (b, r, 32):
        raise RuntimeError(f"raymarch_bwd_camera: g_feat must be [B, R, 32] = [{b}, {r}, 32], got {tuple(g_feat.shape)}")
    d_c2w = torch.empty(b, 16, device=dev, dtype=torch.float32) if reduce else None
    d_intr = torch.empty(b, 9, device=dev, dtype=torch.float32) if reduce else None
    ray_grad = torch.empty(b, r, 6, device=dev, dtype=torch.float32)
    if b == 0:
        return d_c2w, d_intr, ray_grad
    a.g_feat, a.rec = _ptr(g_feat), _ptr(rec)
    L.check(L.lib().hfagp_raymarch_bwd_camera(C.byref(a), _ptr(ray_grad), _ptr(d_c2w), _ptr(d_intr), _stream()),
            "raymarch_bwd_camera")
    return d_c2w, d_intr, ray_grad


def raymarch_rays_bwd(g_feat: Optional[torch.Tensor], planes: torch.Tensor, ray_origins: torch.Tensor, ray_directions: torch.Tensor,
                      u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1, ray_start: float, ray_end: float, box_warp: float,
                      decoder_lr_mul: float = 1.0, plane_axes: int = 0, white_back: bool = False, return_rec: bool = False,
                      decoder_grads: bool = False, decoder_precision: str = "f16x3", planes_absmax: Optional[torch.Tensor] = None,
                      state: Optional[torch.Tensor] = None, rows: Optional[bool] = None, dec_out=None, _out=None,
                      g_depth: Optional[torch.Tensor] = None, g_wsum: Optional[torch.Tensor] = None,
                      depth_range: Optional[torch.Tensor] = None, rec_out: Optional[list] = None,
                      t_near: Optional[torch.Tensor] = None, t_far: Optional[torch.Tensor] = None,
                      g_weights: Optional[torch.Tensor] = None):
    """`raymarch_bwd` of `raymarch_rays`: g_feat [B,R,32] (and / or g_depth, g_wsum [B,R]) → d planes [B,3,H,W,32], with the same
    keywords and return forms.  ``rows``: None = sort + gather whenever it applies, False = the scatter kernels (the image-column
    variant of the grid is not offered for a list).  The sort's scratch is bounded by `rows_scratch_cap()` as for the grid; a list may
    be cut at any ray, so a call that needs more runs in frame chunks and, where one frame is too much, in ray chunks of a frame.
    ``rec_out``: receives pass 1's records [B,R,Sc+Sf,4] (`raymarch_rays_bwd_rays` reads them).  ``t_near`` / ``t_far`` [B,R]: the
    forward call's per-ray limits (hfagp_raymarch_rays_limits_bwd); they carry no gradient, an empty ray contributes exactly zero
    and its g_depth / g_wsum are not read; ``depth_range`` is then `ops.depth_range(tminmax, empty_rays=True)`.
    ``g_weights`` [B,R,Sc+Sf−1]: the gradient w.r.t. the sample_weights of `raymarch_rays(..., samples=True)`, one more addend of the
    compositing adjoint (hfagp_raymarch_rays_samples_bwd); alone it is a sufficient upstream gradient (g_feat None), the records
    carry it on to `raymarch_rays_bwd_rays`, and a chunked call slices it with its rays."""
    who = "raymarch_rays_bwd"
    b, _, _ = _planes_dims(who, planes)
    r = ray_origins.shape[1] if ray_origins.dim() == 3 else -1
    _check_upstream(who, b, r, g_feat, g_depth, g_wsum, depth_range)
    sc, sf = u_strat.shape[-1], u_imp.shape[-1]
    if g_weights is not None and _chk(g_weights, f"{who}: g_weights").shape != (b, r, sc + sf - 1):
        raise RuntimeError(f"{who}: g_weights must be [B, R, Sc + Sf - 1] = [{b}, {r}, {sc + sf - 1}], got {tuple(g_weights.shape)}")
    d_planes, rec = _out if _out is not None else (
        torch.zeros_like(planes), torch.empty(b, max(r, 0), sc + sf, 4, device=planes.device, dtype=torch.float32))
    if rec_out is not None:
        rec_out.append(rec)
    if rows is None:
        rows = os.environ.get("HFAGP_RAYBWD_ROWS", "1") != "0"
    dec = _raymarch_rays_bwd_chunk(
        g_feat=g_feat, planes=planes, ray_origins=ray_origins, ray_directions=ray_directions, u_strat=u_strat,
        u_imp=u_imp.reshape(b, r, sf) if r >= 0 and u_imp.numel() == b * r * sf else u_imp, state=state, g_depth=g_depth, g_wsum=g_wsum,
        g_weights=g_weights, t_near=t_near, t_far=t_far, depth_range=depth_range, d_planes=d_planes, rec=rec, decoder_grads=decoder_grads, dec_out=dec_out,
        rows=rows, dec_w0=dec_w0, dec_b0=dec_b0, dec_w1=dec_w1, dec_b1=dec_b1, ray_start=ray_start, ray_end=ray_end, box_warp=box_warp,
        decoder_lr_mul=decoder_lr_mul, plane_axes=plane_axes, white_back=white_back, decoder_precision=decoder_precision,
        planes_absmax=_decoder_bound(planes, decoder_precision, planes_absmax) if planes.numel() else None)
    if decoder_grads:
        return d_planes, dec
    return (d_planes, rec) if return_rec else d_planes


def _raymarch_rays_bwd_chunk(*, g_feat, planes, ray_origins, ray_directions, u_strat, u_imp, state, g_depth, g_wsum, g_weights,
                             t_near, t_far, depth_range, d_planes, rec, decoder_grads, dec_out, rows, **scene):
    """`raymarch_rays_bwd` of the rays it is given: the whole list or — from itself — a chunk of it (`_raymarch_bwd_frames` for a
    list; u_imp arrives as [B,R,Sf]).  Fills ``d_planes`` and ``rec`` in place, returns the decoder-gradient tuple or None."""
    who = "raymarch_rays_bwd"
    a = L.RayListBwdArgs()
    b, h, w, r, sc, sf, lim = _ray_list_args(who, a, planes, ray_origins, ray_directions, u_strat, u_imp, state=state, t_near=t_near,
                                             t_far=t_far, **scene)
    dec = _dec_grad_out(who, a.bwd, [scene[k] for k in _DEC], decoder_grads, dec_out)
    if b * r == 0:
        return dec
    a.bwd.g_feat, a.bwd.d_planes, a.bwd.rec = _ptr(g_feat), _ptr(d_planes), _ptr(rec)
    scratch = None
    if rows:
        fa = L.RayListArgs()
        fa.base, fa.R = a.bwd.fwd, r
        need = int(L.lib().hfagp_raymarch_rays_bwd_rows_bytes(C.byref(fa)))
        cap, scratch = _rows_scratch(who, a.bwd, need, planes.device, b * r > 1, f"{h} x {w} planes")
        if cap is not None:
            # every per-ray input / output is [B, R, ...]: frames are contiguous slices, and so are the rays r0:r1 of ONE frame; the
            # decoder gradients accumulate in the one `dec`, d_planes accumulates per frame, the depth range is the call's
            per_ray = dict(g_feat=g_feat, ray_origins=ray_origins, ray_directions=ray_directions, u_strat=u_strat, u_imp=u_imp,
                           state=state, g_depth=g_depth, g_wsum=g_wsum, g_weights=g_weights, rec=rec, t_near=t_near, t_far=t_far)
            fit = max(1, int(b * r * cap // need))            # rays one call can take
            nb, nr = (max(1, min(b - 1, fit // r)), r) if fit >= r and b > 1 else (1, max(1, min(r - 1, fit)))
            chunks = 0
            for b0 in range(0, b, nb):
                for r0 in range(0, r, nr):
                    cut = {k: None if t is None else t[b0:b0 + nb, r0:r0 + nr] for k, t in per_ray.items()}
                    _raymarch_rays_bwd_chunk(**cut, planes=planes[b0:b0 + nb], d_planes=d_planes[b0:b0 + nb], depth_range=depth_range,
                                             decoder_grads=decoder_grads, dec_out=dec, rows=rows, **scene)
                    chunks += 1
            ROWS_STATS.update(bytes=min(need, cap), chunks=chunks, path="rows")
            return dec
    gg = _geom_grads(g_depth, g_wsum, depth_range)
    if g_weights is not None:
        L.check(L.lib().hfagp_raymarch_rays_samples_bwd(C.byref(a), C.byref(lim) if lim is not None else None,
                                                        C.byref(gg) if gg is not None else None, _ptr(g_weights), _stream()), who)
    elif lim is not None:
        L.check(L.lib().hfagp_raymarch_rays_limits_bwd(C.byref(a), C.byref(lim), C.byref(gg) if gg is not None else None, _stream()), who)
    else:
        L.check(L.lib().hfagp_raymarch_rays_bwd(C.byref(a), C.byref(gg) if gg is not None else None, _stream()), who)
    return dec


def raymarch_rays_bwd_rays(g_feat: Optional[torch.Tensor], planes: torch.Tensor, rec: torch.Tensor, ray_origins: torch.Tensor,
                           ray_directions: torch.Tensor, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1, ray_start: float,
                           ray_end: float, box_warp: float, decoder_lr_mul: float = 1.0, plane_axes: int = 0, white_back: bool = False,
                           decoder_precision: str = "f16x3", planes_absmax: Optional[torch.Tensor] = None,
                           t_near: Optional[torch.Tensor] = None, t_far: Optional[torch.Tensor] = None):
    """The rays' gradient of `raymarch_rays` (hfagp_raymarch_rays_bwd_rays) → (d origins, d directions), each [B,R,3].  ``g_feat`` and
    the other arguments as in the `raymarch_rays_bwd` call that wrote ``rec`` (its ``rec_out=`` / ``return_rec=True``): the depth,
    opacity and white_back terms are already in the records.  Independent of the pass-2 form that call ran; one writer per ray, no
    atomics: two calls return the same bits.  ``t_near`` / ``t_far``: as in that call (hfagp_raymarch_rays_limits_bwd_rays) — the
    derivative is the one with the limits HELD FIXED, and exactly zero for an empty ray."""
    who = "raymarch_rays_bwd_rays"
    a = L.RayListBwdArgs()
    b, _, _, r, sc, sf, lim = _ray_list_args(who, a, planes, ray_origins, ray_directions, u_strat, u_imp, dec_w0, dec_b0, dec_w1, dec_b1,
                                             ray_start, ray_end, box_warp, decoder_lr_mul, plane_axes, white_back, decoder_precision,
                                             planes_absmax, None, t_near, t_far)
    if _chk(rec, f"{who}: rec").shape != (b, r, sc + sf, 4):
        raise RuntimeError(f"{who}: rec must be [B, R, Sc + Sf, 4] = [{b}, {r}, {sc + sf}, 4], got {tuple(rec.shape)}")
    if g_feat is not None and _chk(g_feat, f"{who}: g_feat").shape != (b, r, 32):
        raise RuntimeError(f"{who}: g_feat must be [B, R, 32] = [{b}, {r}, 32], got {tuple(g_feat.shape)}")
    d_o = torch.empty(b, r, 3, device=planes.device, dtype=torch.float32)
    d_d = torch.empty(b, r, 3, device=planes.device, dtype=torch.float32)
    if b * r == 0:
        return d_o, d_d
    a.bwd.g_feat, a.bwd.rec = _ptr(g_feat), _ptr(rec)
    if lim is not None:
        L.check(L.lib().hfagp_raymarch_rays_limits_bwd_rays(C.byref(a), C.byref(lim), _ptr(d_o), _ptr(d_d), _stream()), who)
    else:
        L.check(L.lib().hfagp_raymarch_rays_bwd_rays(C.byref(a), _ptr(d_o), _ptr(d_d), _stream()), who)
    return d_o, d_d


# ----------------------------------------------------------------------------- loss side of the fitting step
class PoolMSE(torch.autograd.Function):
    """(mean((real - AdaptiveAvgPool2d(size)(img))^2), pooled image) in one pass over `img` [B,C,H,W] (H, W integer
    multiples of real's h, w); backward = one pass writing d img.  The pooled image is returned for the caller's
    book-keeping (the reference returns it from gen_update) and carries no gradient."""

    @staticmethod
    def forward(ctx, img: torch.Tensor, real: torch.Tensor):
        _chk(img, "img"), _chk(real, "real")
        b, c, hh, ww = img.shape
        h, w = real.shape[-2:]
        f = hh // h
        if real.shape[:2] != (b, c) or hh != f * h or ww != f * w or f < 1:
            raise RuntimeError(f"pool_mse: image {tuple(img.shape)} is not an integer multiple of real {tuple(real.shape)}")
        pooled = torch.empty_like(real)
        loss = torch.empty((), device=img.device, dtype=torch.float32)
        ws = torch.empty(L.lib().hfagp_pool_mse_workspace_bytes() // 4, device=img.device, dtype=torch.float32)
        L.check(L.lib().hfagp_pool_mse_fwd(_ptr(img), _ptr(real), _ptr(pooled), _ptr(loss), _ptr(ws), b * c, h, w, f,
                                           _stream()), "pool_mse_fwd")
        ctx.save_for_backward(pooled, real)
        ctx.shape = (b, c, hh, ww, f)
        ctx.mark_non_differentiable(pooled)
        return loss, pooled

    @staticmethod
    def backward(ctx, g_loss, _g_pooled):
        pooled, real = ctx.saved_tensors
        b, c, hh, ww, f = ctx.shape
        d_img = torch.empty(b, c, hh, ww, device=pooled.device, dtype=torch.float32)
        L.check(L.lib().hfagp_pool_mse_bwd(_ptr(pooled), _ptr(real), _ptr(g_loss.contiguous().float()), _ptr(d_img), b * c,
                                           real.shape[-2], real.shape[-1], f, _stream()), "pool_mse_bwd")
        return d_img, None


def pool_mse(img: torch.Tensor, real: torch.Tensor):
    """→ (l2 loss scalar, pooled image [B,C,h,w])."""
    return PoolMSE.apply(img, real)


class PoolWMSE(torch.autograd.Function):
    """`PoolMSE` under a per-pixel weight [B,1,h,w] at the loss resolution, normalised per frame (hfagp_pool_wmse_fwd / _bwd):
    loss = mean over frames of sum(weight (real - pooled)^2) / (C sum(weight)), a frame without weight contributing 0.  One pass
    over `img` forward, one write pass backward, no atomics, no host sync; the pooled image is returned unmasked and carries no
    gradient; there is no gradient w.r.t. `weight` or `real`."""

    @staticmethod
    def forward(ctx, img: torch.Tensor, real: torch.Tensor, weight: torch.Tensor):
        _chk(img, "img"), _chk(real, "real")
        b, c, hh, ww = img.shape
        h, w = real.shape[-2:]
        f = hh // h
        if real.shape[:2] != (b, c) or hh != f * h or ww != f * w or f < 1:
            raise RuntimeError(f"pool_wmse: image {tuple(img.shape)} is not an integer multiple of real {tuple(real.shape)}")
        _chk_operand("pool_wmse", "weight", weight, (b, 1, h, w), img)
        pooled = torch.empty_like(real)
        loss = torch.empty((), device=img.device, dtype=torch.float32)
        inv_d = torch.empty(b, device=img.device, dtype=torch.float32)
        ws = torch.empty(L.lib().hfagp_pool_wmse_workspace_bytes(b) // 4, device=img.device, dtype=torch.float32)
        L.check(L.lib().hfagp_pool_wmse_fwd(_ptr(img), _ptr(real), _ptr(weight), _ptr(pooled), _ptr(loss), _ptr(inv_d), _ptr(ws),
                                            b, c, h, w, f, _stream()), "pool_wmse_fwd")
        ctx.save_for_backward(pooled, real, weight, inv_d)
        ctx.shape = (b, c, hh, ww, f)
        ctx.mark_non_differentiable(pooled)
        return loss, pooled

    @staticmethod
    def backward(ctx, g_loss, _g_pooled):
        pooled, real, weight, inv_d = ctx.saved_tensors
        b, c, hh, ww, f = ctx.shape
        d_img = torch.empty(b, c, hh, ww, device=pooled.device, dtype=torch.float32)
        L.check(L.lib().hfagp_pool_wmse_bwd(_ptr(pooled), _ptr(real), _ptr(weight), _ptr(inv_d), _ptr(g_loss.contiguous().float()),
                                            _ptr(d_img), b, c, real.shape[-2], real.shape[-1], f, _stream()), "pool_wmse_bwd")
        return d_img, None, None


def pool_wmse(img: torch.Tensor, real: torch.Tensor, weight: torch.Tensor):
    """→ (weighted l2 loss scalar, pooled image [B,C,h,w]).  `weight` [B,1,h,w]: float32, contiguous, on the device, finite and
    >= 0 (values above 1 allowed), no gradient.  Where the weight is 0 the pixel is skipped by a branch: NaN / inf in `img` or
    `real` there reach neither the loss nor d img, which is exactly +0.0 there.  Negative or non-finite weights are NOT checked
    (a check would need a host sync): the loss value is then undefined."""
    if not isinstance(weight, torch.Tensor):
        raise TypeError(f"pool_wmse: weight must be a tensor, got {type(weight).__name__}")
    if weight.requires_grad:
        raise RuntimeError("pool_wmse: weight requires grad, and the loss has no gradient w.r.t. the weight; pass weight.detach()")
    return PoolWMSE.apply(img, real, weight)


# ----------------------------------------------------------------------------- optimiser of the fitting step
class AdamTables:
    """Device tables of hfagp_adam_step for one set of (param, grad, exp_avg, exp_avg_sq, step) tensors; built once per set."""

    def __init__(self, params, grads, exp_avgs, exp_avg_sqs, steps):
        chunk = L.lib().hfagp_adam_chunk()
        rows, chunks = [], []
        for k, (p, g, m, v, st) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs, steps)):
            for t in (p, g, m, v):
                if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                    raise RuntimeError("adam_step: fp32 contiguous CUDA tensors only")
            n = p.numel()
            rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), n])
            chunks.extend([k, e] for e in range(0, n, chunk))
        dev = params[0].device
        self.tensors = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self.n, self.nchunks = len(rows), len(chunks)
        self.keep = (list(params), list(grads), list(exp_avgs), list(exp_avg_sqs), list(steps))     # (the pointers stay valid)


def adam_step(tables: AdamTables, lr: float, beta1: float, beta2: float, eps: float) -> None:
    L.check(L.lib().hfagp_adam_step(_ptr(tables.tensors), _ptr(tables.chunks), tables.n, tables.nchunks, lr, beta1, beta2, eps,
                                    _stream()), "adam_step")

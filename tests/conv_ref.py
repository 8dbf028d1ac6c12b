"""float64 reference of the conv GEMM entry points (hfagp_modconv_fwd, hfagp_upconv_fir_fwd, hfagp_torgb_skip_fwd), the emulation
of their 16-bit operand split, a predictor of the kernel a call runs, and the cases their tests share.

Plain torch on the CPU, written from the contracts in include/hfagp.h ("modulated conv", "Weight images"), the tap tables of
csrc/modconv_plan.h and the split of csrc/split_mfma.h; nothing here calls `hfa_gp_amd.ops`, and nothing calls F.conv2d
(tests/test_conv_ref_cpu.py compares with it as the independent formulation).  tests/test_gpu_conv_kernels.py holds the kernels to it.

Every function returns `(value, magnitude)` with the meaning of tests/backward_ref.py.  Tiers:

  exact      `Draw` integers and dyadic scalars: every product of 16-bit parts and every partial sum is an fp32 number, so every
             kind, loop and split-K order must equal the reference bit for bit.
  multipart  exact too, but the operands NEED their low parts: per kind and per part product it keeps (`SUBTIERS`), inputs whose
             values equal the sum of their stored parts, whose tested part is non-zero in a stated share of elements, and whose
             dropped products are identically zero (`multipart_precondition`, through `parts`).
  realistic  randn inputs, per-sample style magnitudes 1e-2 .. 1e2: |got - ref| <= (N + 16) u mag + e_kind mag (+ the absolute
             step of fp16 parts), `kind_bound`; every constant is derived below, none is measured.
"""
import math

import torch

from tests.backward_ref import F64, Draw, U, _d, bound, exact_precondition, f32, worst_ratio  # noqa: F401  (re-exported)
from tests.forward_ref import (ABSMAX_SLOTS, ABSMAX_STRIDE, TIERS, U16, _act, absmax_of, f16_in_normal_range,  # noqa: F401
                               skip_upsample_add, upfir_epilogue, worst_ratio_f16)

MODES = ("3x3", "up", "1x1", "3x3_bwd", "s2_bwd")            # HFAGP_CONV3X3, _CONVT3X3_UP2, _CONV1X1, _CONV3X3_BWD, _CONVS2_BWD
MODE_ID = {m: i for i, m in enumerate(MODES)}
FUSED = ("3x3", "1x1", "3x3_bwd")                            # modes with the epilogue; the other two write raw sums
KINDS = ("f16", "bf16x3", "bf16x6", "f16x3", "f16x2")        # operand kinds 1 .. 5 of split_mfma.h
KINDS16 = ("fp32",) + KINDS
NUM_CU = 256                                                 # kNumCU (csrc/common.h)
F16_MIN_NORMAL = 2.0 ** -14


# ----------------------------------------------------------------------------- the reference
def _taps(mode):
    """(dy, dx, ty, tx) of csrc/modconv_plan.h: the output at (p, q) reads the input at (p + dy, q + dx) with weight tap (ty, tx)."""
    if mode == "1x1":
        return [(0, 0, 0, 0)]
    if mode == "3x3":
        return [(ty - 1, tx - 1, ty, tx) for ty in range(3) for tx in range(3)]
    assert mode == "3x3_bwd"
    return [(ty - 1, tx - 1, 2 - ty, 2 - tx) for ty in range(3) for tx in range(3)]


def _gemm(xa, wa, mode):
    """The bare sum of one mode over already modulated activations xa and the weight wa [Cout, Cin, k, k] the image was made of."""
    co = wa.shape[0]
    if mode in ("3x3", "1x1", "3x3_bwd"):
        b, h, w, _ = xa.shape
        xp = torch.nn.functional.pad(xa, (0, 0, 1, 1, 1, 1))
        acc = torch.zeros(b, h, w, co, dtype=F64)
        for dy, dx, ty, tx in _taps(mode):
            acc += torch.einsum("bhwi,oi->bhwo", xp[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], wa[:, :, ty, tx])
        return acc
    if mode == "up":                  # y_t[2i + ti][2j + tj] += x[i][j] w[ti][tj]
        b, h, w, _ = xa.shape
        acc = torch.zeros(b, 2 * h + 2, 2 * w + 2, co, dtype=F64)
        for ti in range(3):
            for tj in range(3):
                acc[:, ti:ti + 2 * h:2, tj:tj + 2 * w:2] += torch.einsum("bhwi,oi->bhwo", xa, wa[:, :, ti, tj])
        return acc[:, :2 * h + 1, :2 * w + 1].contiguous()
    assert mode == "s2_bwd"           # dx[i][j] = sum g_yt[2i + ti][2j + tj] w[ti][tj], g_yt as its parity images
    _, _, b, h1, w1, _ = xa.shape
    h, w = h1 - 1, w1 - 1
    acc = torch.zeros(b, h, w, co, dtype=F64)
    for ti in range(3):
        for tj in range(3):
            src = xa[ti & 1, tj & 1][:, (ti >> 1):(ti >> 1) + h, (tj >> 1):(tj >> 1) + w]
            acc += torch.einsum("bhwi,oi->bhwo", src, wa[:, :, ti, tj])
    return acc


def modulated(x, styles, mode, batch=None):
    """x * styles per sample and channel in float64; a [1, ...] x is broadcast over `batch` samples (x_batch_stride 0)."""
    x = _d(x)
    bdim = 2 if mode == "s2_bwd" else 0
    if batch is not None and x.shape[bdim] == 1:
        x = x.expand(*x.shape[:bdim], batch, *x.shape[bdim + 1:])
    if styles is None:
        return x
    s = _d(styles)
    return x * (s[None, None, :, None, None, :] if mode == "s2_bwd" else s[:, None, None, :])


def modconv(x, weight, mode, styles=None, dcoef=None, noise=None, strength=0.0, bias=None, act="linear", alpha=0.2, gain=1.0,
            clamp=None, batch=None):
    """hfagp_modconv_fwd: modes '3x3', '1x1', '3x3_bwd': act(sum * dcoef + bias + noise * strength) * gain, clamped;
    'up' (raw [B,2H+1,2W+1,Cout]) and 's2_bwd' (x = parity images [2,2,B,H+1,W+1,Cin]): the bare sums, no epilogue."""
    xs, wa = modulated(x, styles, mode, batch), _d(weight)
    acc, macc = _gemm(xs, wa, mode), _gemm(xs.abs(), wa.abs(), mode)
    if mode not in FUSED:
        return acc, macc
    if dcoef is not None:
        d = _d(dcoef)[:, None, None, :]
        acc, macc = acc * d, macc * d.abs()
    if bias is not None:
        acc, macc = acc + _d(bias), macc + _d(bias).abs()
    if noise is not None:
        nz = _d(noise)[None, :, :, None] * strength
        acc, macc = acc + nz, macc + nz.abs()
    return _act(acc, macc, act, alpha, gain, clamp)


def fused_torgb(y, my, rgb_w):
    """The fused toRGB sums of HfagpModconvArgs::rgb_w [B,3,Cout] over the FINAL y: ([B,H,W,3], magnitude)."""
    r = _d(rgb_w)
    return torch.einsum("bhwo,bro->bhwr", _d(y), r), torch.einsum("bhwo,bro->bhwr", _d(my), r.abs())


def upconv_fir(x, weight, styles=None, dcoef=None, noise=None, strength=0.0, bias=None, act="lrelu", alpha=0.2,
               gain=math.sqrt(2.0), clamp=None, batch=None):
    """hfagp_upconv_fir_fwd = modconv('up') + forward_ref.upfir_epilogue; the magnitude of the raw sums goes through the same map."""
    yt, mt = modconv(x, weight, "up", styles, batch=batch)
    kw = dict(dcoef=dcoef, noise=noise, strength=strength, bias=bias, act=act, alpha=alpha, gain=gain, clamp=clamp)
    return upfir_epilogue(yt, **kw)[0], upfir_epilogue(mt, **kw)[1]


def torgb_skip(x, weight, styles, bias, img=None, plane_major=False):
    """hfagp_torgb_skip_fwd = modconv('1x1', linear, bias) + forward_ref.skip_upsample_add."""
    y, my = modconv(x, weight, "1x1", styles, bias=bias)
    return skip_upsample_add(img, y, plane_major)[0], skip_upsample_add(img, my, plane_major)[1]


def parity_images(g):
    """[B,2H+1,2W+1,C] -> the four parity images [2,2,B,H+1,W+1,C] of hfagp_upfir_bwd's layout (zero beyond)."""
    b, hh, ww, c = g.shape
    p = torch.nn.functional.pad(g, (0, 0, 0, 1, 0, 1))
    return p.reshape(b, (hh + 1) // 2, 2, (ww + 1) // 2, 2, c).permute(2, 4, 0, 1, 3, 5).contiguous()


# ----------------------------------------------------------------------------- the operand split (csrc/split_mfma.h)
NPARTS_A = {"f16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 2, "f16x2": 1}
NPARTS_B = {"f16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 2, "f16x2": 2}
# part products in issue order (A part, B part): kind_pa / kind_pb
PRODUCTS = {"f16": ((0, 0),), "f16x2": ((0, 0), (0, 1)), "f16x3": ((0, 0), (1, 0), (0, 1)), "bf16x3": ((0, 0), (1, 0), (0, 1)),
            "bf16x6": ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2))}


def is_f16(kind):
    return kind in ("f16", "f16x3", "f16x2")


def parts(v, kind, n):
    """n successive round-to-nearest-even 16-bit residuals of the fp32 tensor v, as fp32 tensors: split4<> and the weight-prep
    kernels.  float16 for the fp16 kinds (saturating at +-65504, as split4), bfloat16 otherwise.  v is the operand AFTER the
    kernel's power-of-two scales (`guard`, `image_exponent`)."""
    v = v.float()
    out, r = [], v.clone()
    for _ in range(n):
        p = r.clamp(-65504.0, 65504.0).half().float() if is_f16(kind) else r.bfloat16().float()
        out.append(p)
        r = r - p
    return out


def image_exponent(w, kind):
    """weight_image_exp: e of a scaled float16 image, 8 floor((ex + 3) / 8) for max |w| = f 2^ex, f in [0.5, 1); 0 for bfloat16."""
    m = float(_d(w).abs().max())
    if not is_f16(kind) or not (0.0 < m < 3.0e38):
        return 0
    return max(-120, min(120, 8 * math.floor((math.frexp(m)[1] + 3) / 8)))


def guard(styles_row, kind, x_absmax=None):
    """style_range_guard of one sample: the exponent e whose 2^-e scales the modulated activations of the fp16 kinds (0: the
    bfloat16 kinds carry no guard).  styles_row None: the styles are 1."""
    if not is_f16(kind):
        return 0
    m = 1.0 if styles_row is None else float(_d(styles_row).abs().max())
    e, ex = 0, 15
    if 0.0 < m < 3.0e38:
        e = math.frexp(m)[1]
    if x_absmax is not None and 0.0 < x_absmax < 3.0e38:
        ex = math.frexp(x_absmax)[1]
    return max(-100, min(100, e + ex - 15))


def operand_parts(t, kind, mode, x_absmax=None):
    """(A parts, B parts) as the kernels store them: fp32(x * s) * 2^-e per sample split into NPARTS_A, w * 2^-ew into NPARTS_B."""
    x, s, w = t["x"].float(), t.get("styles"), t["weight"].float()
    bdim = 2 if mode == "s2_bwd" else 0
    nb = x.shape[bdim] if s is None else s.shape[0]
    a = modulated(x, s, mode, nb).float()             # (exact and multipart tiers: the fp32 product is exact, asserted by the caller)
    assert torch.equal(a.double(), modulated(x, s, mode, nb)), "x * styles is not an fp32 number"
    scale = torch.tensor([2.0 ** -guard(None if s is None else s[b], kind, x_absmax) for b in range(nb)], dtype=torch.float32)
    a = a * (scale[None, None, :, None, None, None] if mode == "s2_bwd" else scale[:, None, None, None])
    return (a, parts(a, kind, NPARTS_A[kind])), (w, parts(w * 2.0 ** -image_exponent(w, kind), kind, NPARTS_B[kind]))


def normal_parts(ps, kind, what=""):
    """Every non-zero stored part is a NORMAL number of its type (fp16 subnormals in the matrix pipe: not measured, kept out)."""
    low = F16_MIN_NORMAL if is_f16(kind) else 2.0 ** -126
    for i, p in enumerate(ps):
        nz = p.abs()[p != 0]
        assert nz.numel() == 0 or nz.min().item() >= low, f"{what}: part {i} holds {nz.min().item():.3e}, subnormal"


# sub-tiers of the multipart tier: name -> (A parts needed, B parts needed, the product under test)
SUBTIERS = {
    "f16x3": {"A2xB1": (2, 1, (1, 0)), "A1xB2": (1, 2, (0, 1))},
    "bf16x3": {"A2xB1": (2, 1, (1, 0)), "A1xB2": (1, 2, (0, 1))},
    "f16x2": {"A1xB2": (1, 2, (0, 1))},
    "bf16x6": {"A2xB2": (2, 2, (1, 1)), "A3xB1": (3, 1, (2, 0)), "A1xB3": (1, 3, (0, 2))},
    "f16": {},
}
MIN_SHARE = 0.02          # of the NON-ZERO elements of an operand carry a non-zero tested part (ties that round down leave none)


def multipart_precondition(t, kind, sub, mode, what=""):
    """The operands equal the sum of their stored parts, the tested product is non-zero somewhere on both sides in a stated share
    of the non-zero elements, and every product the kind drops is identically zero."""
    na, nb, (pa, pb) = SUBTIERS[kind][sub]
    (a, ap), (w, bp) = operand_parts(t, kind, mode)
    ew = image_exponent(w, kind)
    assert torch.equal(sum(p.double() for p in ap), a.double()), f"{what}: an activation is not the sum of its parts"
    assert torch.equal(sum(p.double() for p in bp) * 2.0 ** ew, w.double()), f"{what}: a weight is not the sum of its parts"
    normal_parts(ap + bp, kind, what)
    for side, ps, need, tested in (("A", ap, na, pa), ("B", bp, nb, pb)):
        for i, p in enumerate(ps):
            if i >= need:
                assert not p.any(), f"{what}: {side} part {i} must be zero in sub-tier {sub}"
        nz = ps[0] != 0
        share = (ps[tested] != 0).sum().item() / max(1, nz.sum().item())
        assert share >= (MIN_SHARE if tested else 0.5), f"{what}: {side} part {tested} is non-zero in {share:.3f} of the non-zero elements"
    kept = set(PRODUCTS[kind])
    for i in range(len(ap)):
        for j in range(len(bp)):
            if (i, j) not in kept:
                assert not ap[i].any() or not bp[j].any(), f"{what}: the dropped product a{i}b{j} is not identically zero"


# ----------------------------------------------------------------------------- the realistic tier's bound
# e_kind: the relative error of ONE product a b as the kind forms it, to first order, from the contract (hfagp.h, split_mfma.h).
# A type with t significant bits (float16: t = 11, bfloat16: t = 8, the hidden bit included) has the spacing 2^(e - t + 1) in
# [2^e, 2^(e+1)), so round-to-nearest leaves |a - a0| <= 2^(e - t) <= 2^-t |a|.  The residual rho = a - a0 is smaller than 2^(e - t)
# in absolute value unless it is that power of two itself (then it is stored exactly), so it lies in a binade of exponent
# <= e - t - 1 and ITS rounding leaves at most 2^(e - 2t - 1): the residual's sign buys one bit.  By induction, after n parts
#     |a - sum of parts| <= R(n) |a|,   R(n) = 2^-(n (t + 1) - 1)      (float16: 2^-11, 2^-23;  bfloat16: 2^-8, 2^-17, 2^-26)
# and part i >= 1, the rounding of a residual, is at most R(i) |a| in size (part 0: (1 + 2^-t) |a|).  With A kept to na parts and B
# to nb parts:
#     |a b - sum of kept products| <= (R(na) + R(nb)) |a b|  +  sum over the DROPPED products a_i b_j of R(i) R(j) |a b|   (+ 2nd order)
#   f16     na = nb = 1, nothing dropped:                      2 * 2^-11                          = 2^-10
#   f16x2   na = 1, nb = 2, nothing dropped:                   2^-11 + 2^-23
#   f16x3   na = nb = 2, a1 b1 dropped:                        2 * 2^-23 + 2^-22                  = 2^-21
#   bf16x3  na = nb = 2, a1 b1 dropped:                        2 * 2^-17 + 2^-16                  = 2^-15
#   bf16x6  na = nb = 3, a1 b2, a2 b1, a2 b2 dropped:          2 * 2^-26 + 2 * 2^-25 + 2^-34      = 3 * 2^-25 + 2^-34
#   fp32    exact products (v_mfma_f32_32x32x2_f32):           0
# (hfagp.h quotes the typical sizes: ~2^-16, ~2^-23, ~2^-22.)
# The factor (1 + 2^-7) covers the second-order terms: part 0 is up to (1 + 2^-t) |a| on either side, (1 + 2^-8)^2 < 1 + 2^-7, and
# the residual x residual products are below 2^-16 of the first-order sum.
# fp16 STORAGE of x (x_f16): x is read as stored (no rounding), the style is rounded to fp16 and the product x s is a packed fp16
# multiply: the A side costs 2 * 2^-11 instead of 2^-11.
def _res(t_bits, n):
    return 1.0 if n == 0 else 2.0 ** -(n * (t_bits + 1) - 1)


def e_kind(kind, x_f16=False):
    if kind == "fp32":
        return 0.0
    t_bits, na, nb = 11 if is_f16(kind) else 8, NPARTS_A[kind], NPARTS_B[kind]
    kept = set(PRODUCTS[kind])
    e = _res(t_bits, na) + _res(t_bits, nb) + sum(_res(t_bits, i) * _res(t_bits, j) for i in range(na) for j in range(nb)
                                                  if (i, j) not in kept)
    if x_f16:
        e += 2.0 ** -11
    return e * (1.0 + 2.0 ** -7)


def terms(mode, cin):
    """N of the bound: the terms summed into one output, the up-conv's phase with most taps, + 3 for the epilogue."""
    return {"3x3": 9, "3x3_bwd": 9, "1x1": 1, "up": 4, "s2_bwd": 9}[mode] * cin + 3


def kind_bound(t, kind, mode, mag_gemm, x_absmax=None, x_f16=False):
    """The REPRESENTATION part of the bound of the bare GEMM sums, per output element: e_kind mag + the ABSOLUTE step of fp16 parts
    (the summation part, (N + 16) u of the magnitude of the finished output, is added once, by `full_bound`).
    A float16 part below 2^-14 has the absolute step 2^-24, i.e. an error of up to 2^-25 whatever the value: for the weight image
    that is 2^-25 2^ew per element ("the low part's step 2^-24", split_mfma.h; at most 2^-21 max |w|), for the activations
    2^-25 2^e of the sample's guard.  Each enters multiplied by the other operand's absolute value, summed like the GEMM."""
    cin = t["weight"].shape[1]
    bnd = e_kind(kind, x_f16) * mag_gemm
    if kind != "fp32" and is_f16(kind):
        s, w = t.get("styles"), _d(t["weight"])
        nb = mag_gemm.shape[0]
        xs = modulated(t["x"], s, mode, nb).abs()
        step_a = torch.tensor([2.0 ** (guard(None if s is None else s[b], kind, x_absmax) - 25) for b in range(nb)], dtype=F64)
        step_a = step_a[None, None, :, None, None, None] if mode == "s2_bwd" else step_a[:, None, None, None]
        step_w = 2.0 ** (image_exponent(w, kind) - 25)
        bnd = bnd + _gemm(torch.ones_like(xs) * step_a, w.abs(), mode) + _gemm(xs, torch.full_like(w, step_w), mode)
    return bnd


def epilogue_bound(bnd, dcoef=None, gain=1.0):
    """A bound of the GEMM sums behind the epilogue: times |dcoef| and |gain| (lrelu and clamp have slope at most 1)."""
    if dcoef is not None:
        bnd = bnd * _d(dcoef).abs()[:, None, None, :]
    return bnd * abs(gain)


def full_bound(rep, mag, n):
    """rep (the representation bound, carried to the output) + (n + 16) u mag: ONE summation term over everything added into an
    output, n counted by the caller (conv terms + 3 for the epilogue, + the FIR's or the skip's own terms where they follow)."""
    return rep + (n + 16) * U * _d(mag)


def saturated_share(ref, clamp):
    """Share of the outputs that sit ON the clamp: those equal the reference whatever the K loop summed."""
    return 0.0 if clamp is None else (_d(ref).abs() == clamp).double().mean().item()


def ratio(got, ref, bnd):
    """max |got - ref| / bound over all elements (0 / 0 counts as 0)."""
    err = (_d(got) - _d(ref)).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bnd).max().item() if err.numel() else 0.0


# ----------------------------------------------------------------------------- which kernel runs (csrc/modconv_plan.h)
def _span(length, rp):
    return (length + rp - 2) // rp + 1


def plan(c, env=None):
    """The launch of one hfagp_modconv_fwd call, restated from make_plan / resolve_modconv / launch_modconv_bf16: dict(route, ksplit,
    ws_bytes, fringe, up_ns).  c: dict(mode, kind, B, H, W, Cin, Cout) + optional ksplit (0), x_f16, y_f16, rgb, bcast; env: the
    developer switches in force."""
    env = env or {}
    on = lambda k: env.get(k) == "1"             # noqa: E731
    mode, kind, b, h, w, cin, cout = (c[k] for k in ("mode", "kind", "B", "H", "W", "Cin", "Cout"))
    ksplit, x16, y16, rgb = c.get("ksplit", 0), c.get("x_f16", False), c.get("y_f16", False), c.get("rgb", False)
    f32k = kind == "fp32"
    nchunks = cin // (8 if f32k else 16)
    bn = 128 if (cout % 128 == 0 or not f32k) else 96 if cout % 96 == 0 else 64 if cout % 64 == 0 else 32
    tiles_n = -(-cout // bn)
    up, s2 = mode == "up", mode == "s2_bwd"
    gh, gw = (h + 1, w + 1) if up else (h, w)
    ho, wo = (2 * h + 1, 2 * w + 1) if up else (h, w)
    nphase, nslab = (4, 1) if up else (4, 4) if s2 else (1, 1)
    slab = b * ho * wo * cout
    merged_up, merged_s2 = up and not f32k, s2 and not f32k
    if merged_s2:
        nslab = 1
    out = dict(fringe=False, up_ns=0, up_waves=0)
    # the small-image kernel (smallconv_takes)
    if (not f32k and ksplit <= 0 and mode in FUSED and h * w <= (1024 if mode == "1x1" else 256)
            and not (mode != "1x1" and h * w >= 64 and b * h * w >= 1024) and cin % 16 == 0 and cin <= 512 and cout % 32 == 0
            and not x16 and not y16 and not rgb):
        tiles = b * ((h * w + 31) // 32) * ((cout + 31) // 32)
        ks = max(1, min(NUM_CU // tiles, max(1, nchunks // 8)))
        return dict(out, route=f"small/{kind}/taps{1 if mode == '1x1' else 9}", ksplit=ks, ws_bytes=ks * slab * 4 if ks > 1 else 0)
    if merged_up:
        x_stride = 0 if c.get("bcast") else h * w * cin
        fits = lambda ns: ns <= 8 and (ns <= 1 or ns * x_stride * (2 if x16 else 4) < 1 << 32)       # noqa: E731
        rp = -1 if on("HFAGP_DEV_UP_LEGACY_TILES") else h + 1
        fr = rp > 0 and w % 16 == 0 and not on("HFAGP_DEV_UP_NO_FRINGE")
        ns = min(b, max(_span(9, rp), _span(65, rp) if fr else 1)) if rp > 0 else 99
        if not fits(ns) and fr:
            fr, ns = False, min(b, _span(9, rp))
        if not fits(ns):
            rp, fr, ns = (h + 1 + 7) // 8 * 8, False, min(b, 2)
        rows = b * rp
        tr, tw = (rows + 7) // 8, (w // 16) if fr else (w + 1 + 15) // 16
        nf = (rows + 63) // 64 if fr else 0
        waves = 8 if (env.get("HFAGP_DEV_UP_WAVES") == "8" and cout % 128 == 0) else 4
        base = (tr * tw + nf) * (cout // (128 if waves == 8 else 64))
        out.update(fringe=fr, up_ns=ns, up_waves=waves)
    else:
        base = (-(-gh // 8)) * (-(-gw // 16)) * b * tiles_n * (1 if merged_s2 else nphase)
    ks = ksplit
    if ks <= 0:
        ks = max(1, NUM_CU // base) if base < NUM_CU else 1
        ks = min(ks, max(1, nchunks // 2), 64)
    ks = min(ks, nchunks)
    out.update(ksplit=ks, ws_bytes=ks * nslab * slab * 4 if ks * nslab > 1 else 0)
    if f32k:
        return dict(out, route=f"fp32/bn{bn}")
    io = int(x16) | (int(y16) << 1)
    if merged_up:
        loop32 = (out["up_waves"] == 4 and not on("HFAGP_DEV_UP_LEGACY_LOOP") and kind == "f16x3" and not io and cin % 32 == 0
                  and cin <= 512 and cout % 64 == 0)
        waves8 = out["up_waves"] == 8 and kind != "bf16x6"
        return dict(out, route="up/loop32" if loop32 else f"up/{kind}/w{8 if waves8 else 4}/io{io}")
    if merged_s2:
        return dict(out, route=f"s2/{kind}")
    if io:
        return dict(out, route="staged16/f16/taps9/io3")
    epi = "/epi_legacy" if (mode == "3x3" and kind == "f16x3" and on("HFAGP_DEV_CONV_EPILOGUE_LEGACY")) else ""
    if (not on("HFAGP_DEV_CONV9_LEGACY") and kind == "f16x3" and mode == "3x3" and cin % 32 == 0 and cin <= 512 and cout % 128 == 0):
        return dict(out, route="conv9/loop32" + epi)
    return dict(out, route=f"staged16/{kind}/taps{1 if mode == '1x1' else 9}" + epi)


def route(c, env=None):
    return plan(c, env)["route"]


# every kernel instantiation launch_modconv_bf16, launch_smallconv and the fp32 switch can launch in a default or switched process.
# modconv_bf16_kernel<KD, 2, 4> and <KD, 2, 2> (launch_group, 4 and 2 taps) are NOT here: every 16-bit up-conv and its adjoint is
# merged (make_plan: merged_up / merged_s2 for any shape), so no call reaches them.
ROUTES = tuple(
    [f"fp32/bn{bn}" for bn in (128, 96, 64, 32)]
    + [f"staged16/{k}/taps{t}" for k in KINDS for t in (9, 1)] + ["staged16/f16x3/taps9/epi_legacy", "staged16/f16/taps9/io3"]
    + ["conv9/loop32", "conv9/loop32/epi_legacy", "up/loop32"]
    + [f"up/{k}/w4/io0" for k in KINDS] + [f"up/{k}/w8/io0" for k in KINDS if k != "bf16x6"]
    + ["up/f16/w4/io2", "up/f16/w4/io3", "up/f16/w8/io2", "up/f16/w8/io3"]
    + [f"s2/{k}" for k in KINDS] + [f"small/{k}/taps{t}" for k in KINDS for t in (9, 1)])
CHILD_ONLY = tuple(r for r in ROUTES if "/w8/" in r)          # reached under HFAGP_DEV_UP_WAVES=8 only: tests/conv_child.py


# ----------------------------------------------------------------------------- cases
# exact tier: 2^11, a level the integer sums seldom reach (`saturated_share`); it is met exactly where it is planted
CLAMP = {"exact": 2048.0, "realistic": 1.5}
MAX_SATURATED = 0.05


def case(group, mode, kind, B, H, W, Cin, Cout, **kw):
    c = dict(group=group, mode=mode, kind=kind, B=B, H=H, W=W, Cin=Cin, Cout=Cout, ksplit=0, x_f16=False, y_f16=False, rgb=False,
             bcast=False, env={}, epi=7, act="lrelu", clamp=False)
    c.update(kw)
    c["id"] = "{group}-{mode}-{kind}-B{B}x{H}x{W}-{Cin}to{Cout}-ks{ksplit}-e{epi}{act}{clamp:d}".format(**c) + "".join(
        f"-{k}" for k in ("x_f16", "y_f16", "rgb", "bcast") if c[k]) + "".join(f"-{k[10:]}={v}" for k, v in sorted(c["env"].items()))
    return c


def cases():
    """The modconv cases of tests/test_gpu_conv_kernels.py, group by group (the groups of its docstring)."""
    cs = []
    # fp32 staged kernel: the four N tiles, Cin 8 and 24 (1 and 3 chunks of 8), the five modes, ksplit 1 and forced 3, broadcast x
    for cout, cin in ((128, 8), (96, 24), (64, 24), (36, 8), (36, 24)):
        for mode in MODES:
            for ks in (1, 3):
                cs.append(case("fp32", mode, "fp32", 2, 9, 17, cin, cout, ksplit=ks))
    cs.append(case("fp32", "3x3", "fp32", 3, 4, 4, 24, 64, ksplit=1, bcast=True))
    # 16-bit staged, 16-channel loop: every kind; Cin 16 and 48; H x W 1x1, 3x5, 8x16, 9x17; ksplit 1, 2, 7 (> the chunks)
    shapes = ((1, 1, 16, 1), (3, 5, 48, 2), (8, 16, 16, 7), (9, 17, 48, 1), (9, 17, 48, 2), (3, 5, 16, 7), (8, 16, 48, 7))
    for kind in KINDS:
        for mode, cout in (("3x3", 128), ("1x1", 96), ("3x3_bwd", 128), ("s2_bwd", 128)):
            for h, w, cin, ks in shapes:
                cs.append(case("staged16", mode, kind, 2, h, w, cin, cout, ksplit=ks))
    # 32-channel loops (f16x3): one chunk, a pair, a pair + the odd tail; ksplit 1, 2, 3; the legacy switches; fused toRGB
    for mode in ("3x3", "up"):
        for cin in (32, 64, 96):
            for ks in (1, 2, 3):
                cs.append(case("loop32", mode, "f16x3", 2, 9, 17, cin, 128, ksplit=ks))
        leg = "HFAGP_DEV_CONV9_LEGACY" if mode == "3x3" else "HFAGP_DEV_UP_LEGACY_LOOP"
        cs.append(case("loop32", mode, "f16x3", 2, 9, 17, 96, 128, ksplit=2, env={leg: "1"}))
        cs.append(case("loop32", mode, "f16x3", 2, 9, 17, 96, 128, ksplit=1, x_absmax=True))
    cs.append(case("loop32", "3x3", "f16x3", 2, 9, 17, 96, 128, ksplit=1, env={"HFAGP_DEV_CONV_EPILOGUE_LEGACY": "1"}))
    cs.append(case("loop32", "3x3", "f16x3", 2, 9, 17, 96, 128, ksplit=1,
                   env={"HFAGP_DEV_CONV_EPILOGUE_LEGACY": "1", "HFAGP_DEV_CONV9_LEGACY": "1"}))
    for store_y in (True, False):
        cs.append(case("loop32", "3x3", "f16x3", 2, 9, 17, 64, 128, ksplit=1, rgb=True, store_y=store_y))
    cs.append(case("loop32", "3x3", "f16x3", 2, 9, 17, 64, 128, ksplit=1, y_absmax=True))
    # small-image kernel: 4x4 and 5x7 (3x3 and its adjoint), 19x19 (1x1), Cout 32 and 96, one K slice; Cin 256: two slices
    for kind in KINDS:
        for mode, h, w in (("3x3", 4, 4), ("3x3_bwd", 5, 7), ("3x3", 5, 7), ("3x3_bwd", 4, 4), ("1x1", 19, 19)):
            for cout, cin in ((32, 48), (96, 16)):
                cs.append(case("small", mode, kind, 2, h, w, cin, cout))
        cs.append(case("small", "3x3", kind, 1, 4, 4, 256, 32))
        cs.append(case("small", "1x1", kind, 1, 5, 7, 256, 32))
    # merged up-conv: W % 16 == 0 (fringe tiles) and not; a tile over three samples (B 5, H 4); more samples than up_ns; B 9 at H 4:
    # the fringe tiles would stage 9 samples (> 8) and are refused; Cout 64 and 128; fp16 storage
    for kind in KINDS:
        for b, h, w, cin, cout in ((2, 9, 16, 16, 128), (2, 9, 17, 48, 64), (5, 4, 16, 16, 64), (5, 4, 17, 16, 128), (9, 4, 16, 16, 64)):
            cs.append(case("up", "up", kind, b, h, w, cin, cout, ksplit=1))
        cs.append(case("up", "up", kind, 2, 9, 17, 48, 128, ksplit=2))
    cs.append(case("up", "up", "f16", 5, 4, 16, 16, 128, ksplit=1, y_f16=True))
    cs.append(case("up", "up", "f16", 2, 9, 17, 48, 128, ksplit=1, x_f16=True, y_f16=True))
    cs.append(case("up", "3x3", "f16", 2, 9, 17, 48, 128, ksplit=1, x_f16=True, y_f16=True))
    # the epilogue of the fused modes, dealt over the cases in order: dcoef, noise and bias each present and absent (8 masks), the
    # linear activation on every third case, the clamp on every fifth only — a clamped output equals the reference whatever was
    # summed, so the bulk runs without (conv_ref.saturated_share).  fp16 storage of y: no operands, linear, no clamp, so that
    # every output (an even integer below 4096) is a float16 number.
    fused = [c for c in cs if c["mode"] in FUSED]
    for i, c in enumerate(fused):
        kw = dict(epi=0, act="linear", clamp=False) if c["y_f16"] else dict(epi=i % 8, act=("lrelu", "lrelu", "linear")[i % 3], clamp=i % 5 == 0)
        fused[i] = case(**{k: v for k, v in dict(c, **kw).items() if k != "id"})
    it = iter(fused)
    return [next(it) if c["mode"] in FUSED else c for c in cs]


def epilogue_of(c, dr):
    """The epilogue operands of one fused-mode case: bit 0 of c['epi'] dcoef, bit 1 noise, bit 2 bias."""
    if c["mode"] not in FUSED:
        return {}
    b, h, w, cout = c["B"], c["H"], c["W"], c["Cout"]
    kw = dict(act=c["act"], alpha=dr.alpha, gain=dr.gain, clamp=CLAMP[dr.tier] if c["clamp"] else None, strength=dr.strength)
    if c["epi"] & 1:
        kw["dcoef"] = dr.dcoef(b, cout)
    if c["epi"] & 2:
        kw["noise"] = dr.t(h, w)
    if c["epi"] & 4:
        kw["bias"] = dr.t(cout)
    return kw


def _seed(c):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c["id"])) % (1 << 30)


def inputs(c, tier):
    """(tensors of one case: x, weight [Cout, Cin, k, k], styles + the epilogue operands of `modconv`; quantum of the exact tier).
    exact: x, styles, weight integers in [-2, 2] (fp16 storage: [-1, 1]), sample b's styles times 2^(b mod 3) so that the range
    guard's scale differs from sample to sample; the pre-activation values 0, +clamp / gain and
    -clamp / gain (clamp off: +-2) are planted at sample 0, pixel (0, 0), channels 0, 1, 2 of the fused modes, through one
    weight tap of an otherwise zeroed window.
    realistic: randn, styles randn * 10^u, u uniform in [-2, 2] per sample; the clamp, where on, scales with the styles.
    In both tiers at most MAX_SATURATED of the outputs of a clamped case sit on the clamp (tests/test_conv_ref_cpu.py)."""
    b, h, w, cin, cout, mode = (c[k] for k in ("B", "H", "W", "Cin", "Cout", "mode"))
    half = c["x_f16"] or c["y_f16"]
    dr = Draw(tier, _seed(c), r=1 if half else 2)
    k = 1 if mode == "1x1" else 3
    xb = 1 if c["bcast"] else b
    x = dr.t(2, 2, xb, h + 1, w + 1, cin) if mode == "s2_bwd" else dr.t(xb, h, w, cin)
    t = dict(x=x, weight=dr.t(cout, cin, k, k), styles=dr.t(b, cin))
    if tier == "realistic":
        t["styles"] = t["styles"] * (10.0 ** (torch.rand(b, 1, generator=dr.g) * 4.0 - 2.0))
        t["weight"] = t["weight"] * f32(1.0 / math.sqrt(cin * k * k))
    else:                                                # sample b's styles times 2^(b mod 3): every sample its own guard scale
        t["styles"] = t["styles"] * (2.0 ** (torch.arange(b) % 3).float())[:, None]
    t.update(epilogue_of(c, dr))
    if tier == "realistic" and t.get("clamp") is not None:       # ~ four times (1 + the largest sample's style scale): it bites on few outputs
        t["clamp"] = f32(4.0 * (1.0 + float(t["styles"].abs().amax(1).max()) / 3.0))
    if c["rgb"]:
        t["rgb_w"] = dr.t(b, 3, cout, r=1) if dr.exact else dr.t(b, 3, cout) * f32(1.0 / math.sqrt(cout))
    if dr.exact and mode in FUSED and not c["bcast"]:
        target = CLAMP["exact"] / dr.gain if c["clamp"] else 2.0
        x[0, 0:2, 0:2, :] = 0.0                          # the window of output pixel (0, 0)
        x[0, 0, 0, 0], t["styles"][0, 0] = 1.0, 1.0
        ctr = k // 2
        t["weight"][0, 0, ctr, ctr], t["weight"][1, 0, ctr, ctr], t["weight"][2, 0, ctr, ctr] = 0.0, target, -target
        if "dcoef" in t:
            t["dcoef"][0, 0:3] = 1.0
        if "noise" in t:
            t["noise"][0, 0] = 0.0
        if "bias" in t:
            t["bias"][0:3] = 0.0
    # sums of integers; dcoef in halves; noise * strength in halves; lrelu 1/4; gain 2
    return t, 0.5 * 0.25


def planted(c, ref):
    """The planted pre-activation values came out: 0, +target, -target through lrelu, gain and clamp."""
    if c["mode"] not in FUSED or c["bcast"]:
        return
    dr = Draw("exact", 0)
    target = CLAMP["exact"] / dr.gain if c["clamp"] else 2.0
    neg = -target * (dr.alpha if c["act"] == "lrelu" else 1.0) * dr.gain
    assert ref[0, 0, 0, 0].item() == 0.0 and ref[0, 0, 0, 1].item() == target * dr.gain, c["id"]
    assert ref[0, 0, 0, 2].item() == (max(neg, -CLAMP["exact"]) if c["clamp"] else neg), c["id"]


def ref_kwargs(t):
    return {k: v for k, v in t.items() if k not in ("rgb_w",)}


# -- multipart
def multipart_fits(c, sub):
    """Whether a case's K fits the sub-tier: the three-part values span 18 bits, so at most 63 non-zero terms per output may
    meet; the sparse draw below keeps about 14, any K.  Only fp16 storage, the fused toRGB and the one-pixel image (32 activations:
    too few for a share of them to mean anything) are left to the exact tier."""
    return sub in SUBTIERS.get(c["kind"], {}) and not (c["x_f16"] or c["y_f16"] or c["rgb"] or c["bcast"]) and c["H"] * c["W"] > 1


def multipart_inputs(c, sub):
    """(x, weight, styles) of one sub-tier, and the quantum.  Two-part values: i + j 2^-t, i, j in [-1, 1], t = 11 (fp16) or 8
    (bfloat16): 1 + 2^-t is a tie that rounds to 1 and leaves the residual 2^-t.  Three-part values (bf16x6): +-m 2^-17, m an
    18-bit integer in [2^17, 2^18).  The one-part side: integers in [-1, 1].  Styles: +-1 and +-0.5 where one side is one-part and
    the other two-part (one +-1 per sample: the guard's scale is then 2^-1), +-1 otherwise.  Sparse operands where the sums
    would leave fp32: the many-part side keeps a seeded share of its elements (the positions differ from case to case)."""
    kind, mode = c["kind"], c["mode"]
    b, h, w, cin, cout = (c[k] for k in ("B", "H", "W", "Cin", "Cout"))
    na, nb, _ = SUBTIERS[kind][sub]
    g = torch.Generator().manual_seed(_seed(c) + 17 * na + nb)
    k = 1 if mode == "1x1" else 3
    t_bits = 11 if is_f16(kind) else 8
    nterms = {"3x3": 9, "3x3_bwd": 9, "1x1": 1, "up": 4, "s2_bwd": 9}[mode] * cin
    xshape = (2, 2, b, h + 1, w + 1, cin) if mode == "s2_bwd" else (b, h, w, cin)

    def draw(shape, n):
        i = torch.randint(-1, 2, shape, generator=g).double()
        if n == 1:
            return i
        if n == 2:
            return i + torch.randint(-1, 2, shape, generator=g).double() * 2.0 ** -t_bits
        m = torch.randint(2 ** 17, 2 ** 18, shape, generator=g).double() * 2.0 ** -17
        return m * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)

    x, wt = draw(xshape, na), draw((cout, cin, k, k), nb)
    heavy = na + nb >= 4                                   # bf16x6: quantum 2^-16 (A2xB2) or 2^-17 (three parts)
    if heavy:
        keep = min(1.0, (40.0 if na == nb else 20.0) / nterms)
        if na >= nb:
            x = x * (torch.rand(xshape, generator=g) < keep)
        else:
            wt = wt * (torch.rand(cout, cin, k, k, generator=g) < keep)
    s = torch.randint(0, 2, (b, cin), generator=g).double() * 2 - 1
    q = 2.0 ** -(16 if na == nb else 17) if heavy else 2.0 ** -t_bits
    if not heavy:
        s = s * (1.0 - 0.5 * torch.randint(0, 2, (b, cin), generator=g).double())
        s[:, 0] = 1.0
        q = q / 2
    return dict(x=x.float(), weight=wt.float(), styles=s.float()), q


# ----------------------------------------------------------------------------- hfagp_upconv_fir_fwd, hfagp_torgb_skip_fwd
FIR_SHAPES = {"strip": (2, 9, 20, 48, 128), "lean": (2, 9, 20, 32, 128), "strip32": (2, 9, 20, 32, 128)}      # (B, H, W, Cin, Cout)
FIR_ENV = {"strip": {"HFAGP_DEV_FIR_MIN_BLOCKS": "1"}, "lean": {"HFAGP_DEV_FIR_MIN_BLOCKS": "1", "HFAGP_DEV_FIR_LEAN": "1"},
           "strip32": {"HFAGP_DEV_FIR_MIN_BLOCKS": "1", "HFAGP_DEV_FIR_LEAN": "0"}}
FIR_CLAMP_EXACT = 256.0                                  # met exactly where it is planted; the filtered sums seldom reach it
FIR_KINDS = ("f16", "bf16x3", "f16x3", "f16x2")           # (bf16x6 is refused: fuse_plan; f16x2 runs as f16x3, hfagp.h)


def fir_cases(kernel):
    """Eight epilogue combinations per kernel and kind: dcoef, noise, bias each present and absent; both activations and the
    clamp on and off alternate over them."""
    b, h, w, cin, cout = FIR_SHAPES[kernel]
    for kind in FIR_KINDS:
        for mask in range(8):
            yield case("fir_" + kernel, "up", kind, b, h, w, cin, cout, epi=mask, act=("lrelu", "linear")[(mask >> 1) & 1],
                       clamp=bool((mask ^ (mask >> 2)) & 1), env=FIR_ENV[kernel])


def fir_multipart(kernel):
    """(case, sub-tier, tensors, quantum) of the multipart tier through the fused layer: one case per kind and sub-tier, no epilogue
    operands, linear, gain 1; the FIR's taps are sixteenths, so the quantum is a sixteenth of `multipart_inputs`'."""
    for c in fir_cases(kernel):
        if c["epi"] == 0:
            for sub in SUBTIERS[c["kind"]]:
                t, q = multipart_inputs(c, sub)
                yield c, sub, dict(t, act="linear", gain=1.0, clamp=None), q / 16


def skip_multipart():
    """(case, sub-tier, tensors, quantum) of the multipart tier through torgb_skip: zero bias, no image, Cout 32 and 96."""
    b, h, w, cin = SKIP_SHAPE
    for c in skip_cases():
        if not c["img"] and not c["plane_major"]:
            for sub in SUBTIERS[c["kind"]]:
                t, q = multipart_inputs(case("skip", "1x1", c["kind"], b, h, w, cin, c["Cout"]), sub)
                yield c, sub, dict(t, bias=torch.zeros(c["Cout"])), q


def fir_inputs(c, tier):
    """As `inputs`, with the epilogue operands of the up-sampling layer on the [2H, 2W] grid; quantum: FIR taps in sixteenths."""
    b, h, w, cin, cout = (c[k] for k in ("B", "H", "W", "Cin", "Cout"))
    dr = Draw(tier, _seed(c), r=2)
    t = dict(x=dr.t(b, h, w, cin), weight=dr.t(cout, cin, 3, 3), styles=dr.t(b, cin))
    if tier == "realistic":
        t["styles"] = t["styles"] * (10.0 ** (torch.rand(b, 1, generator=dr.g) * 4.0 - 2.0))
        t["weight"] = t["weight"] * f32(1.0 / math.sqrt(cin * 9))
    t.update(act=c["act"], alpha=dr.alpha, gain=dr.gain, clamp=(FIR_CLAMP_EXACT if dr.exact else CLAMP[tier]) if c["clamp"] else None,
             strength=dr.strength)
    if tier == "realistic" and t["clamp"] is not None:
        t["clamp"] = f32(4.0 * (1.0 + float(t["styles"].abs().amax(1).max()) / 3.0))
    if c["epi"] & 1:
        t["dcoef"] = dr.dcoef(b, cout)
    if c["epi"] & 2:
        t["noise"] = dr.t(2 * h, 2 * w)
    if c["epi"] & 4:
        t["bias"] = dr.t(cout)
    if dr.exact:
        # planted at sample 0, output pixel (0, 0), channels 0, 1, 2: its FIR window is y_t rows and columns 0 .. 2, fed by
        # x[0:2, 0:2] only.  That window of x is zero but for x[0, 0, channel 0] = 1 (style 1), whose weights are zero but for tap
        # (2, 2), which the FIR weighs with f[3]^2 = 1/16: the pre-activation value is w[co, 0, 2, 2] / 16.
        target = FIR_CLAMP_EXACT / dr.gain
        t["x"][0, 0:2, 0:2, :] = 0.0
        t["x"][0, 0, 0, 0], t["styles"][0, 0] = 1.0, 1.0
        t["weight"][0:3, 0] = 0.0
        t["weight"][1, 0, 2, 2], t["weight"][2, 0, 2, 2] = 16.0 * target, -16.0 * target
        if "dcoef" in t:
            t["dcoef"][0, 0:3] = 1.0
        if "noise" in t:
            t["noise"][0, 0] = 0.0
        if "bias" in t:
            t["bias"][0:3] = 0.0
    return t, (1 / 16) * 0.5 * 0.25


def fir_planted(c, t, ref):
    """The planted pre-activation values 0, +clamp / gain, -clamp / gain came out through lrelu, gain and clamp."""
    target = FIR_CLAMP_EXACT / t["gain"]
    neg = -target * (t["alpha"] if c["act"] == "lrelu" else 1.0) * t["gain"]
    assert ref[0, 0, 0, 0].item() == 0.0 and ref[0, 0, 0, 1].item() == FIR_CLAMP_EXACT, c["id"]
    assert ref[0, 0, 0, 2].item() == (max(neg, -FIR_CLAMP_EXACT) if c["clamp"] else neg), c["id"]


def fir_bound(t, kind, mag_t):
    """Bound of the fused layer: the raw sums' representation bound through the FIR and the epilogue as a magnitude, and one
    summation term with N = 4 Cin (conv) + 16 (FIR taps) + 3 (epilogue) against the finished output's magnitude."""
    kw = {k: t.get(k) for k in ("dcoef", "noise", "bias")}
    run_kind = "f16x3" if kind == "f16x2" else kind
    raw = kind_bound(t, run_kind, "up", mag_t)
    through = upfir_epilogue(raw, dcoef=kw["dcoef"], act="linear", gain=t["gain"])[1]          # (no noise / bias: they carry no error)
    full = upfir_epilogue(mag_t, strength=t["strength"], act="linear", gain=t["gain"], **kw)[1]
    return full_bound(through, full, 4 * t["weight"].shape[1] + 16 + 3)


SKIP_SHAPE = (1, 128, 128, 16)                               # the smallest shape ops.torgb_skip_supported admits
SKIP_KINDS = ("f16", "bf16x3", "bf16x6", "f16x3")


def skip_cases():
    for kind in SKIP_KINDS:
        for cout, plane_major in ((32, False), (96, False), (96, True)):
            for img in (False, True):
                yield dict(kind=kind, Cout=cout, plane_major=plane_major, img=img,
                           id=f"skip-{kind}-{cout}-{'pm' if plane_major else 'cl'}-{'img' if img else 'noimg'}")


def skip_inputs(c, tier):
    b, h, w, cin = SKIP_SHAPE
    dr = Draw(tier, _seed(c), r=2)
    t = dict(x=dr.t(b, h, w, cin), weight=dr.t(c["Cout"], cin, 1, 1), styles=dr.t(b, cin), bias=dr.t(c["Cout"]))
    if tier == "realistic":                              # per-sample style magnitude 1e-2 .. 1e2, by the case: the range guard at both ends
        n = [k["id"] for k in skip_cases()].index(c["id"])
        t["styles"] = t["styles"] * f32(10.0 ** (-2.0 + 4.0 * (n % 5) / 4.0))
        t["weight"] = t["weight"] * f32(1.0 / math.sqrt(cin))
    if c["img"]:
        t["img"] = dr.t(b, h // 2, w // 2, c["Cout"])
    return t, 1 / 16

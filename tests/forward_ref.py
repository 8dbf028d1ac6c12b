"""float64 reference of the forward streaming entry points of csrc/elementwise.hip, and the cases their tests share.

Plain torch on the CPU, written from the contracts in include/hfagp.h and the comments above each kernel in csrc/elementwise.hip;
nothing here calls `hfa_gp_amd.ops` or the library.  tests/test_forward_ref_cpu.py proves every function against an independent
float64 formulation (torch.nn.functional, the oracle); tests/test_gpu_forward_kernels.py holds the kernels to them.

Every function returns `(value, magnitude)` with the meaning of tests/backward_ref.py: the magnitude is the same formula with every
product replaced by its absolute value and every subtraction by an addition, per output element.  lrelu and clamp are continuous
with slope at most 1, so a magnitude passes through them scaled by |gain| only (never clamped, never multiplied by alpha).

The two tiers, `Draw`, `exact_precondition`, `bound` and `worst_ratio` are those of tests/backward_ref.py.
"""
import itertools
import math
import re
from pathlib import Path

import torch

from tests.backward_ref import F64, Draw, U, _d, bound, exact_precondition, f32, worst_ratio  # noqa: F401  (re-exported)

_SRC = Path(__file__).resolve().parents[1] / "hfa-gp_amd" / "csrc" / "elementwise.hip"
K_STRIP = int(re.search(r"#define\s+HFAGP_FIR_STRIP\s+(\d+)", _SRC.read_text()).group(1))     # output rows per thread of the FIR kernel
ABSMAX_SLOTS, ABSMAX_STRIDE = 64, 32                                                          # HFAGP_ABSMAX_SLOTS / _STRIDE
U16 = 2.0 ** -11          # unit roundoff of fp16
F16_MIN_NORMAL, F16_MAX = 2.0 ** -14, 65504.0

_UP = (0.25, 0.75, 0.75, 0.25)         # [1,3,3,1] / 4: the up-sampling FIR per axis (gain 2 per axis folded in)
_DOWN = (0.125, 0.375, 0.375, 0.125)   # [1,3,3,1] / 8: the blur per axis


def _pair(fn, *ts):
    """fn over the operands and over their absolute values."""
    return fn(*ts), fn(*(t.abs() for t in ts))


def _act(pre, mpre, act, alpha, gain, clamp):
    """lrelu (slope alpha below 0), gain, clamp to [-clamp, clamp]; the magnitude is scaled by |gain| only."""
    v = torch.where(pre < 0, pre * alpha, pre) if act == "lrelu" else pre
    v = v * gain
    if clamp is not None and clamp >= 0:
        v = v.clamp(-clamp, clamp)
    return v, mpre * abs(gain)


def _up2_axis(t, dim):
    """upsample2d along one axis: out[2i] = .25 in[i-1] + .75 in[i], out[2i+1] = .75 in[i] + .25 in[i+1], zero beyond."""
    n = t.shape[dim]
    pad = [0, 0] * (t.dim() - 1 - dim) + [1, 1]
    p = torch.nn.functional.pad(t, pad)
    lo, mid, hi = p.narrow(dim, 0, n), p.narrow(dim, 1, n), p.narrow(dim, 2, n)
    out = torch.stack((0.25 * lo + 0.75 * mid, 0.75 * mid + 0.25 * hi), dim=dim + 1)
    shape = list(t.shape)
    shape[dim] = 2 * n
    return out.reshape(shape)


def _up2(t, dims):
    return _up2_axis(_up2_axis(t, dims[0]), dims[1])


# ----------------------------------------------------------------------------- the entry points
def demod(styles, wsq, eps):
    """dcoef [B,Cout] = rsqrt(sum_i styles^2 wsq + eps) of GIVEN styles.  Magnitude: dcoef itself — the argument is a sum of
    non-negative terms, so its relative error is at most (Cin + 3) u, and the inverse square root halves a relative error."""
    arg = _d(styles) ** 2 @ _d(wsq).T + eps
    d = arg ** -0.5
    return d, d.abs()


def styles_demod(w, affine_w, affine_b, wsq=None, style_gain=1.0, eps=1e-8):
    """hfagp_style_fwd / one item of hfagp_style_batch_fwd: ((styles [B,Cin], dcoef [B,Cout] | None), magnitudes);
    styles = (w . A_i / sqrt(w_dim) + b_i) * style_gain, dcoef from those styles."""
    w, a, b = _d(w), _d(affine_w), _d(affine_b)
    wgain = 1.0 / math.sqrt(w.shape[1])
    s, ms = (w @ a.T * wgain + b) * style_gain, (w.abs() @ a.abs().T * wgain + b.abs()) * abs(style_gain)
    if wsq is None:
        return (s, None), (ms, None)
    d, md = demod(s, wsq, eps)
    return (s, d), (ms, md)


def fully_connected(x, weight, bias, lr_mul=1.0, act="linear", alpha=0.2, gain=1.0):
    """hfagp_fc_fwd: act((x . W_o) lr_mul / sqrt(In) + b_o lr_mul) * gain, no clamp."""
    x, wt = _d(x), _d(weight)
    wg = lr_mul / math.sqrt(x.shape[1])
    pre, mpre = x @ wt.T * wg, x.abs() @ wt.abs().T * abs(wg)
    if bias is not None:
        pre, mpre = pre + _d(bias) * lr_mul, mpre + _d(bias).abs() * abs(lr_mul)
    return _act(pre, mpre, act, alpha, gain, None)


def weight_prep(weight):
    """hfagp_weight_prep: ((wt [taps][Cin/4][Cout][4], wsq [Cout][Cin]), magnitudes); wt[t][ci/4][co][ci%4] = w[co][ci][t]."""
    wt = _d(weight)
    co, ci = wt.shape[:2]
    flat = wt.reshape(co, ci // 4, 4, -1)                              # [co][ci/4][ci%4][t]
    img = flat.permute(3, 1, 0, 2).contiguous()
    wsq = (wt.reshape(co, ci, -1) ** 2).sum(-1)
    return (img, wsq), (img.abs(), wsq)


def upfir_epilogue(yt, dcoef=None, noise=None, strength=0.0, bias=None, act="lrelu", alpha=0.2, gain=math.sqrt(2.0), clamp=None):
    """hfagp_upfir_epilogue_fwd: yt [B,2H+1,2W+1,C] (fp32, or fp16 storage read as stored) -> [B,2H,2W,C];
    out[Y][X] = sum_pq f[p] f[q] yt[Y+p-1][X+q-1] (zero beyond), f = [1,3,3,1] / 4, then * dcoef + noise * strength + bias,
    lrelu, gain, clamp.  The value is NOT rounded to the storage type."""
    yt = _d(yt)
    b, hi, wi, c = yt.shape
    ho, wo = hi - 1, wi - 1

    def fir(src):
        p4 = torch.nn.functional.pad(src, (0, 0, 1, 1, 1, 1))
        acc = torch.zeros(b, ho, wo, c, dtype=F64)
        for p in range(4):
            for q in range(4):
                acc += _UP[p] * _UP[q] * p4[:, p:p + ho, q:q + wo]
        return acc

    pre, mpre = _pair(fir, yt)
    if dcoef is not None:
        d = _d(dcoef)[:, None, None, :]
        pre, mpre = pre * d, mpre * d.abs()
    if noise is not None:
        nz = _d(noise)[None, :, :, None] * strength
        pre, mpre = pre + nz, mpre + nz.abs()
    if bias is not None:
        pre, mpre = pre + _d(bias), mpre + _d(bias).abs()
    return _act(pre, mpre, act, alpha, gain, clamp)


def skip_upsample_add(img, y, plane_major=False):
    """hfagp_skip_upsample_add: upsample2d(img [B,H,W,C]) + y [B,2H,2W,C], or y alone; plane_major: [B,3,Ho,Wo,C/3]."""
    y = _d(y)
    o, m = y, y.abs()
    if img is not None:
        up, mup = _pair(lambda t: _up2(t, (1, 2)), _d(img))
        o, m = o + up, m + mup
    if plane_major:
        b, ho, wo, c = o.shape
        o, m = (t.reshape(b, ho, wo, 3, c // 3).permute(0, 3, 1, 2, 4).contiguous() for t in (o, m))
    return o, m


def _torgb_tail(acc, macc, bias, rgb_in, clamp):
    pre, mpre = acc + _d(bias)[None, :, None, None], macc + _d(bias).abs()[None, :, None, None]
    out = pre.clamp(-clamp, clamp) if (clamp is not None and clamp >= 0) else pre
    mout = mpre
    if rgb_in is not None:
        up, mup = _pair(lambda t: _up2(t, (2, 3)), _d(rgb_in))
        out, mout = out + up, mout + mup
    return (out, pre), (mout, mpre)


def torgb_small(x, weight, styles, bias, rgb_in=None, clamp=None):
    """hfagp_torgb_fwd: ((rgb_out, y_pre) NCHW [B,Cout,H,W], magnitudes); y_pre = sum_ci x w s + bias, rgb_out = clamp(y_pre) +
    upsample2d(rgb_in [B,Cout,H/2,W/2])."""
    acc, macc = _pair(lambda a, b, c: torch.einsum("bhwi,oi,bi->bohw", a, b, c), _d(x), _d(weight), _d(styles))
    return _torgb_tail(acc, macc, bias, rgb_in, clamp)


def torgb_finish(part, bias, rgb_in=None, clamp=None):
    """hfagp_torgb_finish_fwd: part [nparts,B,H,W,4] (channel 3 unused) summed over the parts, then as torgb_small."""
    cout = bias.shape[0]
    acc, macc = _pair(lambda p: p.sum(0)[..., :cout].permute(0, 3, 1, 2), _d(part))
    return _torgb_tail(acc, macc, bias, rgb_in, clamp)


def blur_down(x):
    """hfagp_blur_down_fwd: y[i][j] = sum_aq f[a] f[q] x[2i+a-1][2j+q-1], f = [1,3,3,1] / 8, zero beyond; [B,H,W,C] -> [B,H/2,W/2,C]."""
    x = _d(x)
    b, h, w, c = x.shape

    def run(src):
        p1 = torch.nn.functional.pad(src, (0, 0, 1, 1, 1, 1))
        acc = torch.zeros(b, h // 2, w // 2, c, dtype=F64)
        for a in range(4):
            for q in range(4):
                acc += _DOWN[a] * _DOWN[q] * p1[:, a:a + h - 1:2, q:q + w - 1:2]
        return acc
    return _pair(run, x)


def blur_down_bwd(gy):
    """hfagp_blur_down_bwd: the adjoint, gx[2i+a-1][2j+q-1] += f[a] f[q] gy[i][j]; [B,H/2,W/2,C] -> [B,H,W,C]."""
    gy = _d(gy)
    b, ho, wo, c = gy.shape
    h, w = 2 * ho, 2 * wo

    def run(src):
        acc = torch.zeros(b, h + 2, w + 2, c, dtype=F64)
        for a in range(4):
            for q in range(4):
                acc[:, a:a + h - 1:2, q:q + w - 1:2] += _DOWN[a] * _DOWN[q] * src
        return acc[:, 1:h + 1, 1:w + 1].contiguous()
    return _pair(run, gy)


def upfirdn2d(x, f, up=1, down=1, padding=(0, 0, 0, 0), gain=1.0):
    """hfagp_upfirdn2d_fwd on NCHW: zero-insert by `up` (H up x W up samples), pad / crop by (px0, px1, py0, py1), TRUE convolution
    with f [fh, fw] (the filter flipped), decimate by `down`, times gain:
        y[oy][ox] = gain sum_pq f[fh-1-p][fw-1-q] z[oy down + p - py0][ox down + q - px0]."""
    x, f = _d(x), _d(f)
    n, c, h, w = x.shape
    fh, fw = f.shape
    px0, px1, py0, py1 = padding
    ho, wo = (h * up + py0 + py1 - fh) // down + 1, (w * up + px0 + px1 - fw) // down + 1
    big = max(abs(v) for v in padding) + max(fh, fw) + down

    def run(src, flt):
        z = torch.zeros(n, c, h, up, w, up, dtype=F64)
        z[:, :, :, 0, :, 0] = src
        z = torch.nn.functional.pad(z.reshape(n, c, h * up, w * up), (big, big + down * wo, big, big + down * ho))
        acc = torch.zeros(n, c, ho, wo, dtype=F64)
        for p in range(fh):
            for q in range(fw):
                y0, x0 = big + p - py0, big + q - px0
                acc += flt[fh - 1 - p, fw - 1 - q] * z[:, :, y0:y0 + down * ho:down, x0:x0 + down * wo:down]
        return acc
    y, m = run(x, f), run(x.abs(), f.abs())
    return y * gain, m * abs(gain)


def bias_act(x, b=None, dim=1, act="linear", alpha=0.2, gain=1.0, clamp=None):
    """hfagp_bias_act_fwd: bias along `dim`, lrelu, gain, clamp."""
    pre = _d(x)
    mpre = pre.abs()
    if b is not None:
        shape = [1] * pre.dim()
        shape[dim] = -1
        pre, mpre = pre + _d(b).reshape(shape), mpre + _d(b).abs().reshape(shape)
    return _act(pre, mpre, act, alpha, gain, clamp)


def nchw_to_nhwc(x):
    y = _d(x).permute(0, 2, 3, 1).contiguous()
    return y, y.abs()


def nhwc_to_nchw(x):
    y = _d(x).permute(0, 3, 1, 2).contiguous()
    return y, y.abs()


# ----------------------------------------------------------------------------- fp16 storage
def f16_precondition(ref, mag, q, what=""):
    """Exact tier with fp16 storage: on top of `exact_precondition`, the STORED value is a multiple of q below 2^11 q, hence an
    fp16 number."""
    exact_precondition(ref, mag, q, what)
    top = (_d(ref).abs() / q).max().item()
    assert top < 2.0 ** 11, f"{what}: |reference| / quantum = {top:.3e} >= 2^11"
    assert q >= 2.0 ** -24, what


def f16_in_normal_range(ref, what=""):
    """Realistic tier with fp16 storage: every non-zero reference value is a normal fp16 number, so the final rounding costs at
    most 2^-11 |ref|."""
    a = _d(ref).abs()
    assert a.max().item() < F16_MAX, f"{what}: beyond fp16's range"
    nz = a[a > 0]
    assert nz.numel() == 0 or nz.min().item() >= F16_MIN_NORMAL, f"{what}: {nz.min().item():.3e} is subnormal in fp16"


def worst_ratio_f16(got, ref, mag, n):
    """max |got - ref| / ((n + 16) u magnitude + 2^-11 |ref|)."""
    ref = _d(ref)
    err, bnd = (_d(got) - ref).abs(), bound(mag, n) + U16 * ref.abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bnd).max().item()


def absmax_of(slots):
    """The maximum an absmax buffer [HFAGP_ABSMAX_FLOATS] publishes: over its 64 slots, one per 32 floats."""
    return _d(slots).reshape(ABSMAX_SLOTS, ABSMAX_STRIDE)[:, 0].max().item()


# ----------------------------------------------------------------------------- shared cases
CLAMP = {"exact": 4.0, "realistic": 1.5}
TIERS = ("exact", "realistic")

# -- upfir_epilogue
UPFIR_C, UPFIR_B = (4, 12, 64), (1, 2)
UPFIR_HW = ((1, 1), (K_STRIP // 2, 2), (K_STRIP // 2 + 1, 3), (3, 5))      # one pixel pair; exactly one strip; a strip + 2 rows; wide
UPFIR_N = 16 + 3


def upfir_threads(b, h, w, c):
    """Threads of the launch that do work: (sample, strip, column pair, 4 channels)."""
    return b * (-(-2 * h // K_STRIP)) * w * (c // 4)


def upfir_cases(c, hw, half, tier):
    """Every combination of B, dcoef / noise / bias present and absent, act and clamp at one (C, H, W, storage): 64 cases."""
    for b, mask, act, clamp_on in itertools.product(UPFIR_B, range(8), ("linear", "lrelu"), (False, True)):
        yield dict(C=c, H=hw[0], W=hw[1], B=b, half=half, tier=tier, dcoef=bool(mask & 1), noise=bool(mask & 2), bias=bool(mask & 4),
                   act=act, clamp=clamp_on)


def upfir_inputs(case):
    """(kwargs of forward_ref.upfir_epilogue as CPU tensors — yt float16 for fp16 storage —, quantum of the exact tier).  Exact
    tier: three pre-activation values of sample 0, row 0 are planted through one tap of weight 1/16 in an otherwise zeroed
    window: exactly 0 at (X 0, channel 0), exactly +clamp / gain at (X 1, channel 1), exactly -clamp / gain at (X 0, channel 2)."""
    c, h, w, b, half, tier = (case[k] for k in ("C", "H", "W", "B", "half", "tier"))
    seed = 20000 + 1000 * c + 100 * h + 10 * w + b + 7 * (case["dcoef"] + 2 * case["noise"] + 4 * case["bias"]) + 3 * case["clamp"]
    dr = Draw(tier, seed + (500000 if half else 0) + (1 if case["act"] == "lrelu" else 0), r=1 if half else 3)
    yt = dr.t(b, 2 * h + 1, 2 * w + 1, c)
    sign = None
    if half and not dr.exact:         # one sign per case and away from 0: |pre| >= 0.5 * 1.75^2 * 0.5 - 0.1 max |noise| stays a normal fp16 number
        sign = -1.0 if b == 2 else 1.0
        yt = (yt.abs() + 0.5) * sign
    kw = dict(act=case["act"], alpha=dr.alpha, gain=dr.gain, clamp=CLAMP[tier] if case["clamp"] else None, strength=dr.strength)
    if case["dcoef"]:
        kw["dcoef"] = dr.dcoef(b, c)
        if half and dr.exact:
            kw["dcoef"] = kw["dcoef"].clamp(min=1.0)                     # (keeps the fp16 quantum at 1/32)
    if case["noise"]:
        kw["noise"] = dr.t(2 * h, 2 * w)
    if case["bias"]:
        kw["bias"] = dr.t(c) if sign is None else (dr.t(c).abs() + 0.5) * sign
    if dr.exact:
        target = CLAMP[tier] / dr.gain
        d = kw["dcoef"][0] if case["dcoef"] else torch.ones(c)
        yt[0, 0:3, 0:4, 0:3] = 0.0                                      # the windows of (Y 0, X 0) and (Y 0, X 1), channels 0..2
        yt[0, 2, 0, 1] = target * 16.0 / d[1]                           # row 2 = tap p 3, column 0 = tap q 0 of X 1
        yt[0, 2, 2, 2] = -target * 16.0 / d[2]                          # row 2, column 2 = tap q 3 of X 0
        if case["noise"]:
            kw["noise"][0, 0:2] = 0.0
        if case["bias"]:
            kw["bias"][0:3] = 0.0
    kw["yt"] = yt.half() if half else yt
    # fir in 1/16; d >= 1/2 (fp16 storage: >= 1); noise * strength in 1/2; lrelu 1/4; gain 2
    return kw, (1 / 16) * (1.0 if half else 0.5) * 0.25 * 2.0


def upfir_planted(case, ref):
    """The planted values came out: 0, +clamp / gain and -clamp / gain before the activation."""
    if case["tier"] != "exact":
        return
    dr = Draw("exact", 0)
    t = CLAMP["exact"] / dr.gain
    neg = -t * (dr.alpha if case["act"] == "lrelu" else 1.0) * dr.gain
    assert ref[0, 0, 0, 0].item() == 0.0 and ref[0, 0, 1, 1].item() == CLAMP["exact"], case
    assert ref[0, 0, 0, 2].item() == (max(neg, -CLAMP["exact"]) if case["clamp"] else neg), case


# -- skip_upsample_add
SKIP_C, SKIP_IMG, SKIP_B = (4, 12, 96), ((1, 1), (2, 3), (5, 4), None), (1, 2)
SKIP_N = 5


def skip_inputs(c, img_hw, b, tier):
    """(img [B,H,W,C] | None, y): y is [B,2H,2W,C], or [B,3,5,C] without an image.  Quantum 1/16."""
    dr = Draw(tier, 30000 + 100 * c + b + (17 * img_hw[0] + img_hw[1] if img_hw else 0))
    if img_hw is None:
        return None, dr.t(b, 3, 5, c), 1.0
    return dr.t(b, img_hw[0], img_hw[1], c), dr.t(b, 2 * img_hw[0], 2 * img_hw[1], c), 1 / 16


# -- toRGB
TORGB_CIN_LDS, TORGB_CIN_REG = (8, 24, 512), (64, 128, 256)
TORGB_COUT = (1, 2, 3, 4)
TORGB_HW = ((2, 2), (6, 10), (18, 16))            # 4 pixels < one 32-pixel row of a block; 60; 288 = one 256-pixel block + a partial one
TORGB_FLAGS = tuple(itertools.product((False, True), repeat=3))       # rgb_in, clamp, y_pre


def torgb_clamp(cin, tier):
    """A clamp that bites on part of the image: the exact tier's sums grow like sqrt(8 Cin)."""
    return 2.0 * int(math.sqrt(cin)) if tier == "exact" else CLAMP[tier]


def torgb_inputs(cin, cout, hw, b, tier):
    """x [B,H,W,Cin], weight [Cout,Cin], styles [B,Cin] (realistic: of size 1 / sqrt(Cin), as the generator's), bias, rgb_in."""
    dr = Draw(tier, 40000 + 10 * cin + cout + 1000 * hw[0] + b, r=2)
    t = dict(x=dr.t(b, hw[0], hw[1], cin), weight=dr.t(cout, cin), styles=dr.t(b, cin), bias=dr.t(cout, r=4),
             rgb_in=dr.t(b, cout, hw[0] // 2, hw[1] // 2, r=4))
    if not dr.exact:
        t["styles"] = t["styles"] * f32(1.0 / math.sqrt(cin))
    return t, 1 / 16


FINISH_NPARTS, FINISH_COUT = (1, 3), (1, 3)


def finish_inputs(nparts, cout, hw, b, tier):
    dr = Draw(tier, 50000 + 10 * nparts + cout + 1000 * hw[0] + b)
    return dict(part=dr.t(nparts, b, hw[0], hw[1], 4), bias=dr.t(cout), rgb_in=dr.t(b, cout, hw[0] // 2, hw[1] // 2)), 1 / 16


# -- styles
STYLE_WDIM = {"exact": (4, 64), "realistic": (4, 64, 260, 512)}      # exact: 1 / sqrt(w_dim) a power of two; 260 = a 256-wide trip + a tail
STYLE_CIN, STYLE_COUT, STYLE_B = (1, 3, 64, 65, 130), (None, 1, 63, 64, 65), (1, 3)
STYLE_EPS = {"exact": 2.0 ** -10, "realistic": 1e-8}


def style_inputs(wd, cin, cout, b, tier, seed=0):
    """ws [B,3,w_dim] (the kernel is given row 1, contiguous or as the strided view), affine_w, affine_b, wsq | None, style_gain, eps;
    quantum of styles: 1 / sqrt(w_dim) * style_gain (1/4)."""
    dr = Draw(tier, 60000 + 7 * wd + 131 * cin + 17 * (cout or 0) + b + seed)
    t = dict(ws=dr.t(b, 3, wd), affine_w=dr.t(cin, wd), affine_b=dr.t(cin), wsq=None if cout is None else dr.pos(cout, cin),
             style_gain=0.25 if dr.exact else f32(1.0 / math.sqrt(cin)), eps=STYLE_EPS[tier])
    return t, 0.25 / math.sqrt(wd)


def style_batch_items(n, tier):
    """n items of one hfagp_style_batch_fwd call: B * Cin and B * Cout differ from item to item (the grid of the largest overhangs
    the others), every third item has no dcoef (item 1 of 3 lies between two with), w_dim cycles through the tier's values."""
    wds = STYLE_WDIM[tier] if tier == "exact" else (64, 260, 512)
    items = []
    for i in range(n):
        cin, cout, b = STYLE_CIN[(2 * i + 1) % 5], (1, 63, 64, 65)[i % 4], (3, 1, 2)[i % 3]
        wd = wds[i % len(wds)]
        items.append((wd, style_inputs(wd, cin, None if i % 3 == 1 else cout, b, tier, seed=1000 * (i + 1))))
    return items


# -- fully connected
FC_IN = {"exact": (1, 64), "realistic": (1, 63, 64, 65, 512)}
FC_LR = {"exact": 0.5, "realistic": f32(0.01)}


STYLE_PARAMS = [(wd, tier) for tier in TIERS for wd in STYLE_WDIM[tier]]
FC_PARAMS = [(fin, tier) for tier in TIERS for fin in FC_IN[tier]]


def fc_cases():
    return list(itertools.product((1, 5), (1, 3), (False, True), ("linear", "lrelu")))      # Out, B, bias, act


def fc_inputs(fin, fout, b, tier):
    dr = Draw(tier, 70000 + 10 * fin + fout + b)
    return dict(x=dr.t(b, fin), weight=dr.t(fout, fin), bias=dr.t(fout), lr_mul=FC_LR[tier], alpha=dr.alpha, gain=dr.gain), \
        0.5 / math.sqrt(fin) * 0.25


# -- the smaller families
WPREP = ((1, 4, 1), (5, 8, 3), (33, 12, 3), (96, 16, 1))
BLUR_HW, BLUR_C, BLUR_B = ((2, 2), (2, 6), (6, 4)), (4, 12), (1, 2)
UPFIRDN = ((1, 1, (1, 1, 1, 1)), (2, 1, (2, 1, 2, 1)), (1, 2, (1, 1, 1, 1)), (2, 1, (1, 2, 2, 0)), (1, 1, (0, 0, 0, 0)))
TRANSPOSE = ((3, 33), (33, 1), (32, 32), (40, 63))             # (C, H * W)


def upfirdn_filter():
    """3 x 4 dyadic taps, neither square nor symmetric: a flip or a transposition of the filter changes the result."""
    return torch.tensor([[1.0, 2.0, 0.5, 3.0], [0.25, 1.0, 4.0, 1.5], [2.0, 0.125, 1.0, 0.75]]) / 16.0


def upfirdn_inputs(up, down, tier):
    return Draw(tier, 80000 + 10 * up + down).t(2, 3, 9, 7), 2.0 ** -7       # filter in 1/128


def bias_act_inputs(shape, dim, tier, with_bias=True):
    """x with the pre-activation values 0, +clamp / gain, -clamp / gain planted at flat indices 0, 1, 2 (bias subtracted)."""
    dr = Draw(tier, 90000 + dim + len(shape))
    x = dr.t(*shape)
    b = dr.t(shape[dim]) if with_bias else None
    t = CLAMP[tier] / dr.gain
    inner = math.prod(shape[dim + 1:])
    flat = x.view(-1)
    for i, v in enumerate((0.0, t, -t)):
        flat[i] = v - (b[(i // inner) % shape[dim]].item() if with_bias else 0.0)
    return x, b, dr, 0.25

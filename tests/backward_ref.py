"""float64 reference of the backward streaming and weight-gradient entry points, and the cases their tests share.

Plain torch on the CPU, written from the contracts in include/hfagp.h ("backward pass" and "gradients w.r.t. the generator
weights") and from the bookkeeping comment at the top of csrc/backward.hip; nothing here calls `hfa_gp_amd.ops` or the library.
tests/test_backward_ref_cpu.py proves every function against float64 autograd; tests/test_gpu_backward_kernels.py holds the
kernels to them.

Every function returns `(value, magnitude)`.  The magnitude is the same formula with every product term replaced by its absolute
value and every subtraction by an addition, per output element: what a rounding error of the kernel is measured against.

Two tiers of inputs (`Draw`):
  exact      small integers in [-r, r] (r <= 4) and powers of two for every scalar, so that every product and every partial sum
             is exact in fp32 in any order: the kernel must equal the reference bit for bit.  `exact_precondition` asserts what
             that rests on: the reference is a multiple of the case's quantum q (a power of two), and magnitude / q < 2^24.
  realistic  randn inputs; |got - ref| <= (N + 16) * 2^-24 * magnitude for N summed terms (`bound`).
"""
import math
import random

import torch

F64 = torch.float64
U = 2.0 ** -24            # unit roundoff of fp32


def _d(t):
    return None if t is None else t.detach().to("cpu", F64)


def f32(v: float) -> float:
    """The value a `float` field of the C structs holds."""
    return torch.tensor(v, dtype=torch.float32).item()


# ----------------------------------------------------------------------------- the entry points
def pointwise_bwd(x, dxs_conv=None, s_conv=None, dxs_rgb=None, s_rgb=None, g_rgb_small=None, w_rgb_small=None, s_small=None,
                  g_direct=None, producer=None, param_grads=True, y_rgb_small=None, clamp_rgb_small=None, g_nchw3_a=None,
                  g_nchw3_b=None):
    """hfagp_pointwise_bwd: ((g_out [B,H,W,C], sums [B,10,C]), (their magnitudes)).  `producer` as ops.pointwise_bwd takes it
    (`noise_strength_dev`, when present, wins over `noise_strength`)."""
    x = _d(x)
    b, h, w, c = x.shape
    ax = x.abs()
    gx, mx = torch.zeros_like(x), torch.zeros_like(x)
    sums, msums = torch.zeros(b, 10, c, dtype=F64), torch.zeros(b, 10, c, dtype=F64)

    def pix(t):
        return t.sum(dim=(1, 2))

    for row, (g, s) in enumerate(((dxs_conv, s_conv), (dxs_rgb, s_rgb))):
        if g is None:
            continue
        g, s = _d(g), _d(s)[:, None, None, :]
        gx, mx = gx + g * s, mx + (g * s).abs()
        sums[:, row], msums[:, row] = pix(g * x), pix(g.abs() * ax)
    if g_rgb_small is not None:
        gs = _d(g_rgb_small)                                            # NCHW [B,Co,H,W]
        if y_rgb_small is not None and clamp_rgb_small is not None and clamp_rgb_small >= 0:
            gs = gs * (_d(y_rgb_small).abs() < clamp_rgb_small)
        gs = gs.permute(0, 2, 3, 1)                                     # [B,H,W,Co]
        wr, ss = _d(w_rgb_small), _d(s_small)[:, None, None, :]
        t, mt = gs @ wr, gs.abs() @ wr.abs()
        gx, mx = gx + t * ss, mx + mt * ss.abs()
        sums[:, 2], msums[:, 2] = pix(t * x), pix(mt * ax)
        if param_grads:
            for co in range(gs.shape[-1]):
                sums[:, 6 + co], msums[:, 6 + co] = pix(gs[..., co:co + 1] * x), pix(gs[..., co:co + 1].abs() * ax)
    if g_direct is not None:
        gx, mx = gx + _d(g_direct), mx + _d(g_direct).abs()
    for g3 in (g_nchw3_a, g_nchw3_b):
        if g3 is not None:
            g3 = _d(g3).permute(0, 2, 3, 1)
            gx[..., :3] += g3
            mx[..., :3] += g3.abs()
    if producer is None:
        return (gx, sums), (mx, msums)

    gain, alpha, clamp = producer.get("gain", f32(math.sqrt(2.0))), producer.get("alpha", f32(0.2)), producer.get("clamp")
    lrelu = producer.get("act", "lrelu") == "lrelu"
    strength = producer.get("noise_strength", 0.0)
    if producer.get("noise_strength_dev") is not None:
        strength = _d(producer["noise_strength_dev"]).item()
    neg = (~(x > 0)) if lrelu else torch.zeros_like(x, dtype=torch.bool)      # slope alpha AT 0 too
    slope = torch.where(neg, torch.full_like(x, alpha), torch.ones_like(x))
    keep = (ax < clamp) if (clamp is not None and clamp >= 0) else torch.ones_like(x, dtype=torch.bool)
    g_pre, m_pre = gx * gain * slope * keep, mx * abs(gain) * slope.abs() * keep
    d = _d(producer["dcoef"])[:, None, None, :] if producer.get("dcoef") is not None else torch.ones(1, 1, 1, c, dtype=F64)
    bias = _d(producer["bias"]) if producer.get("bias") is not None else torch.zeros(c, dtype=F64)
    noise = _d(producer["noise"])[None, :, :, None] if producer.get("noise") is not None else torch.zeros(1, h, w, 1, dtype=F64)
    pre = x / gain / slope                                              # lrelu^-1(X / gain)
    sums[:, 3] = pix(g_pre * (pre - bias - noise * strength) / d)
    msums[:, 3] = pix(m_pre * (pre.abs() + bias.abs() + (noise * strength).abs()) / d.abs())
    if param_grads:
        sums[:, 4], msums[:, 4] = pix(g_pre), pix(m_pre)
        sums[:, 5], msums[:, 5] = pix(g_pre * noise), pix(m_pre * noise.abs())
    return (g_pre * d, sums), (m_pre * d.abs(), msums)


def style_bwd(ds, dd, styles, dcoef, wsq, affine_w, style_gain=1.0, dw0=None):
    """hfagp_style_bwd / one item of hfagp_style_batch_bwd: ((dstot [B,Cin], dw [B,w_dim]), magnitudes); dw0: the row accumulated
    into (None: overwritten)."""
    ds, styles, a = _d(ds), _d(styles), _d(affine_w)
    acc = macc = torch.zeros_like(ds)
    if dd is not None:
        dd, d3, wsq = _d(dd), _d(dcoef) ** 3, _d(wsq)
        acc, macc = (dd * d3) @ wsq, (dd * d3).abs() @ wsq.abs()
    dstot, mstot = (ds - styles * acc) * style_gain, (ds.abs() + styles.abs() * macc) * abs(style_gain)
    wgain = 1.0 / math.sqrt(a.shape[1])
    dw, mdw = dstot @ a * wgain, mstot @ a.abs() * wgain
    if dw0 is not None:
        dw, mdw = dw + _d(dw0), mdw + _d(dw0).abs()
    return (dstot, dw), (mstot, mdw)


def affine_grad(dstot, w, dA0, db0):
    """hfagp_affine_grad(_batch): ((dA, db), magnitudes), both accumulated into dA0 / db0."""
    dstot, w = _d(dstot), _d(w)
    wgain = 1.0 / math.sqrt(w.shape[1])
    return ((_d(dA0) + dstot.T @ w * wgain, _d(db0) + dstot.sum(0)),
            (_d(dA0).abs() + dstot.abs().T @ w.abs() * wgain, _d(db0).abs() + dstot.abs().sum(0)))


def bias_noise_grads(sums, dbias0=None, dnoise0=None):
    """hfagp_bias_noise_grads: ((dbias | None, dnoise | None), magnitudes) from rows 4 and 5 of sums [B,10,C]."""
    s = _d(sums)
    db = None if dbias0 is None else (_d(dbias0) + s[:, 4].sum(0), _d(dbias0).abs() + s[:, 4].abs().sum(0))
    dn = None if dnoise0 is None else (_d(dnoise0) + s[:, 5].sum(), _d(dnoise0).abs() + s[:, 5].abs().sum())
    return tuple(None if t is None else t[0] for t in (db, dn)), tuple(None if t is None else t[1] for t in (db, dn))


def planes_to_nhwc(pm):
    """hfagp_planes_to_nhwc: plane-major [B,3,H,W,Cp] -> channels-last [B,H,W,3 Cp]."""
    pm = _d(pm)
    b, _, h, w, cp = pm.shape
    y = pm.permute(0, 2, 3, 1, 4).reshape(b, h, w, 3 * cp)
    return y, y.abs()


def bias_act_bwd(dy, y, act, alpha, gain, clamp):
    """hfagp_bias_act_bwd: dx = dy * gain * (y <= 0 ? alpha : 1) where |y| < clamp, else 0, from the forward OUTPUT y."""
    dy, y = _d(dy), _d(y)
    slope = torch.where(~(y > 0), torch.full_like(y, alpha), torch.ones_like(y)) if act == "lrelu" else torch.ones_like(y)
    keep = (y.abs() < clamp) if (clamp is not None and clamp >= 0) else torch.ones_like(y, dtype=torch.bool)
    return dy * gain * slope * keep, dy.abs() * abs(gain) * slope.abs() * keep


_FIR = (0.25, 0.75, 0.75, 0.25)


def upfir_bwd(gy):
    """hfagp_upfir_bwd: g_y [B,2H,2W,C] -> gph [2,2,B,H+1,W+1,C], gph[a][b][m][n] = g_yt[2m+a][2n+b] with
    g_yt[Y][X] = sum_pq f[p] f[q] g_y[Y-p+1][X-q+1] on (2H+1) x (2W+1), zero beyond; f = [1,3,3,1] / 4."""
    gy = _d(gy)
    b, ho, wo, c = gy.shape
    out = []
    for src in (gy, gy.abs()):
        p4 = torch.nn.functional.pad(src, (0, 0, 2, 2, 2, 2))                  # P[Y - p + 1 + 2]
        gyt = torch.zeros(b, ho + 2, wo + 2, c, dtype=F64)
        for p in range(4):
            for q in range(4):
                gyt[:, :ho + 1, :wo + 1] += _FIR[p] * _FIR[q] * p4[:, 3 - p:3 - p + ho + 1, 3 - q:3 - q + wo + 1]
        out.append(gyt.reshape(b, ho // 2 + 1, 2, wo // 2 + 1, 2, c).permute(2, 4, 0, 1, 3, 5).contiguous())
    return out[0], out[1]


def upsample2d_bwd(g, channels_last):
    """hfagp_upsample2d_bwd: g_in[i][j] = sum_pq k[p] k[q] g[2i-1+p][2j-1+q], k = [.25,.75,.75,.25]; [B,2H,2W,C] or [B,C,2H,2W]."""
    g = _d(g)
    if channels_last:
        g = g.permute(0, 3, 1, 2)
    ho, wo = g.shape[2:]
    out = []
    for src in (g, g.abs()):
        p1 = torch.nn.functional.pad(src, (1, 1, 1, 1))
        acc = torch.zeros(*g.shape[:2], ho // 2, wo // 2, dtype=F64)
        for p in range(4):
            for q in range(4):
                acc += _FIR[p] * _FIR[q] * p1[:, :, p:p + ho:2, q:q + wo:2]
        out.append(acc.permute(0, 2, 3, 1).contiguous() if channels_last else acc)
    return out[0], out[1]


def conv_wgrad(x, styles, g, weight, mode, dd=None, dcoef=None, dw0=None):
    """hfagp_conv_wgrad: dweight [Cout,Cin,k,k] = conv-weight-gradient(x * styles, g) - weight * sum_b dd d^3 styles^2 (+ dw0).
    mode '3x3' / '1x1': g [B,H,W,Cout]; 'up': g = the parity images of upfir_bwd, [2,2,B,H+1,W+1,Cout]."""
    x, g, weight = _d(x), _d(g), _d(weight)
    b, h, w, cin = x.shape
    xs = x * _d(styles)[:, None, None, :] if styles is not None else x
    out = []
    for xa, ga in ((xs, g), (xs.abs(), g.abs())):
        dw = torch.zeros_like(weight)
        if mode == "1x1":
            dw[:, :, 0, 0] = torch.einsum("bmni,bmno->oi", xa, ga)
        elif mode == "3x3":
            xp = torch.nn.functional.pad(xa, (0, 0, 1, 1, 1, 1))
            for ty in range(3):
                for tx in range(3):
                    dw[:, :, ty, tx] = torch.einsum("bmni,bmno->oi", xp[:, ty:ty + h, tx:tx + w], ga)
        else:
            for ti in range(3):
                for tj in range(3):
                    gp = ga[ti & 1, tj & 1][:, (ti >> 1):(ti >> 1) + h, (tj >> 1):(tj >> 1) + w]
                    dw[:, :, ti, tj] = torch.einsum("bmni,bmno->oi", xa, gp)
        out.append(dw)
    dw, mdw = out
    if dd is not None:
        dem = (_d(dd) * _d(dcoef) ** 3).T @ _d(styles) ** 2                     # [Cout,Cin]
        mdem = (_d(dd) * _d(dcoef) ** 3).abs().T @ _d(styles) ** 2
        dw, mdw = dw - weight * dem[:, :, None, None], mdw + weight.abs() * mdem[:, :, None, None]
    if dw0 is not None:
        dw, mdw = dw + _d(dw0), mdw + _d(dw0).abs()
    return dw, mdw


# ----------------------------------------------------------------------------- the two bars
def exact_precondition(ref, mag, q, what=""):
    """What bit-for-bit equality of an fp32 kernel with the float64 reference rests on: every term and every partial sum, in any
    order, is a multiple of the power of two q and smaller in absolute value than 2^24 q, hence an fp32 number."""
    ref, mag = _d(ref), _d(mag)
    assert math.log2(q) == round(math.log2(q)), f"{what}: quantum {q} is no power of two"
    assert torch.equal(ref.float().double(), ref), f"{what}: the reference is not an fp32 tensor"
    assert torch.equal((ref / q).round(), ref / q) and torch.equal((mag / q).round(), mag / q), f"{what}: not a multiple of {q}"
    top = (mag / q).max().item() if mag.numel() else 0.0
    assert top < 2.0 ** 24, f"{what}: magnitude / quantum = {top:.3e} >= 2^24"
    assert bool((ref.abs() <= mag).all()), f"{what}: |reference| above its magnitude"


def bound(mag, n):
    """Realistic tier: any-order fp32 summation of n terms, (n - 1) u, plus 17 u for the roundings inside one term, against the
    magnitude (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first order)."""
    return (n + 16) * U * _d(mag)


def worst_ratio(got, ref, mag, n):
    """max |got - ref| / bound over all elements (0 / 0 counts as 0; anything / 0 as inf)."""
    err, bnd = (_d(got) - _d(ref)).abs(), bound(mag, n)
    if err.numel() == 0:
        return 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return ratio.max().item()


# ----------------------------------------------------------------------------- inputs
class Draw:
    """Seeded inputs of one case in one tier; fp32 tensors on the CPU (their float64 images are exact)."""

    def __init__(self, tier: str, seed: int, r: int = 4):
        assert tier in ("exact", "realistic") and 1 <= r <= 4
        self.tier, self.exact, self.r = tier, tier == "exact", r
        self.g = torch.Generator().manual_seed(seed)

    def t(self, *shape, r=None):
        """A general operand: integers in [-r, r] / randn."""
        r = self.r if r is None else r
        if self.exact:
            return torch.randint(-r, r + 1, shape, generator=self.g).float()
        return torch.randn(*shape, generator=self.g)

    def pos(self, *shape):
        """A non-negative operand (sums of squares): integers in [0, r] / rand."""
        if self.exact:
            return torch.randint(0, self.r + 1, shape, generator=self.g).float()
        return torch.rand(*shape, generator=self.g)

    def dcoef(self, *shape):
        """Demodulation coefficients: {0.5, 1, 2} / rand + 0.5."""
        if self.exact:
            return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=self.g)]
        return torch.rand(*shape, generator=self.g) + 0.5

    @property
    def gain(self):
        return 2.0 if self.exact else f32(math.sqrt(2.0))

    @property
    def alpha(self):
        return 0.25 if self.exact else f32(0.2)

    @property
    def strength(self):
        return 0.5 if self.exact else f32(0.1)


# ----------------------------------------------------------------------------- pointwise_bwd cases
PW_C = (12, 32, 96, 512, 1024)          # C/4 = 3 (idle threads), 8 (smallest PACKED), 24, 128 (two waves per pixel), 256 (one pixel lane)
PW_HW = ((1, 1), (3, 5), (17, 23))
PW_CHUNKS = ("default", "one", "hw", "empty")      # empty: 7 chunks at H*W = 15 -> rows of 3, chunks 5 and 6 hold no pixel
PW_CLAMP = {"exact": 4.0, "realistic": 1.5}
PW_CLAMP_SMALL = {"exact": 2.0, "realistic": 1.0}


def pointwise_cases():
    """At most 40 operand combinations (the same list in both tiers).  The first 20 are every kernel variant (SMALL x PG; PACKED
    follows from C) at every C; shapes, chunk counts and optional operands are dealt from a seeded generator, and
    a few combinations are pinned; `pointwise_coverage` asserts that every optional operand and every producer setting occurs
    present and absent, and that the pinned combinations are there."""
    rnd = random.Random(20261018)
    cases = []

    def add(c, small, pg, hw=None, chunks=None, **pin):
        k = len(cases)
        hw = hw or PW_HW[k % 3]
        chunks = chunks or PW_CHUNKS[(k // 3) % 3]
        b = (1, 3)[rnd.random() < 0.5]
        if c * hw[0] * hw[1] * b * 4 > 2 << 20:
            b = 1
        flag = lambda p: rnd.random() < p        # noqa: E731
        case = dict(id=k, C=c, H=hw[0], W=hw[1], B=b, chunks=chunks, small=small, pg=pg,
                    dxs_conv=flag(0.6), dxs_rgb=(not small) and flag(0.6), g_direct=flag(0.5), g_nchw3_a=flag(0.4),
                    g_nchw3_b=flag(0.4), Co=rnd.choice((1, 3, 4)) if small else 0, mask_in_kernel=small and flag(0.5),
                    producer=flag(0.75), dcoef=flag(0.6), bias=flag(0.6), noise=flag(0.6), clamp=flag(0.6),
                    act=("lrelu", "linear")[flag(0.3)], strength_dev=flag(0.4), deferred=flag(0.3))
        case.update(pin)                         # (after the deal: a pin does not shift the other cases)
        cases.append(case)

    for c in PW_C:
        for small in (False, True):
            for pg in (False, True):
                add(c, small, pg)
    # trailing chunks without a pixel; the two PACKED ones with all four small-toRGB channels masked in the kernel (lanes 4 .. 7 of
    # a lane group load y_rgb_small[0 .. 3] for the shuffles) and with the deferred reduction (the partial sums are inspected)
    packed4 = dict(Co=4, mask_in_kernel=True, deferred=True)
    for c, small, pg, pin in ((32, True, False, packed4), (96, True, True, {}), (512, True, True, packed4), (12, False, True, {})):
        add(c, small, pg, hw=(3, 5), chunks="empty", **pin)
    for c, small, pg, hw, chunks in ((1024, True, True, (17, 23), "hw"), (96, False, False, (17, 23), "one"),
                                    (32, True, True, (17, 23), "default"), (12, True, False, (1, 1), "hw"),
                                    (512, False, True, (3, 5), "hw"), (96, True, False, (3, 5), "one"),
                                    (32, False, False, (1, 1), "default"), (1024, False, False, (3, 5), "default")):
        add(c, small, pg, hw=hw, chunks=chunks)
    return cases


def pointwise_variant(case):
    c4 = case["C"] // 4
    return case["small"], case["pg"], case["small"] and c4 >= 8 and c4 & (c4 - 1) == 0


def pointwise_chunks(case):
    """The value of ops._DEV_PW_CHUNKS that forces the case's chunk count (None: the library's default)."""
    hw = case["H"] * case["W"]
    return {"default": None, "one": "1", "hw": str(hw), "empty": "7"}[case["chunks"]]


def pointwise_coverage(cases):
    assert len(cases) <= 40
    for c in PW_C:
        admits = {(s, p, s and (c // 4) >= 8 and (c // 4) & (c // 4 - 1) == 0) for s in (False, True) for p in (False, True)}
        assert {pointwise_variant(k) for k in cases if k["C"] == c} == admits, c
    assert len({pointwise_variant(k) for k in cases}) == 6
    assert {(k["H"], k["W"]) for k in cases} == set(PW_HW) and {k["B"] for k in cases} == {1, 3}
    assert {k["chunks"] for k in cases} == set(PW_CHUNKS)
    assert all((k["H"], k["W"]) == (3, 5) for k in cases if k["chunks"] == "empty")
    for key in ("dxs_conv", "dxs_rgb", "g_direct", "g_nchw3_a", "g_nchw3_b", "small", "pg", "deferred", "producer"):
        assert {bool(k[key]) for k in cases} == {False, True}, key
    assert {k["Co"] for k in cases if k["small"]} == {1, 3, 4}
    assert {k["mask_in_kernel"] for k in cases if k["small"]} == {False, True}
    for pg in (False, True):
        assert any(pointwise_variant(k) == (True, pg, True) and k["Co"] == 4 and k["mask_in_kernel"] for k in cases), pg
    assert any(k["chunks"] == "empty" and k["deferred"] for k in cases)
    prod = [k for k in cases if k["producer"]]
    for key in ("dcoef", "bias", "noise", "clamp", "strength_dev"):
        assert {bool(k[key]) for k in prod} == {False, True}, key
    assert {k["act"] for k in prod} == {"lrelu", "linear"}
    assert any(k["noise"] and k["strength_dev"] and k["pg"] for k in prod)       # row 5 next to a device-side strength


def pointwise_inputs(case, tier):
    """(kwargs of ops.pointwise_bwd / backward_ref.pointwise_bwd as fp32 CPU tensors, quantum of the exact tier).  The caller
    moves the tensors to the device; `producer['noise_strength_dev']` is a 0-d tensor, and the host value next to it is wrong
    on purpose (the device value wins)."""
    b, h, w, c = case["B"], case["H"], case["W"], case["C"]
    dr = Draw(tier, 1000 + case["id"], r=4 if h * w < 100 else 3)
    x = dr.t(b, h, w, c, r=4)
    kw = dict(x=x, param_grads=case["pg"])
    clamp = PW_CLAMP[tier]
    if dr.exact and x.numel() >= 3:                       # planted: the alpha branch at 0 and the clamp mask at +-clamp
        x.view(-1)[0], x.view(-1)[1], x.view(-1)[2] = 0.0, clamp, -clamp
    if case["dxs_conv"]:
        kw.update(dxs_conv=dr.t(b, h, w, c), s_conv=dr.t(b, c))
    if case["dxs_rgb"]:
        kw.update(dxs_rgb=dr.t(b, h, w, c), s_rgb=dr.t(b, c))
    if case["small"]:
        co, cs = case["Co"], PW_CLAMP_SMALL[tier]
        gs, y = dr.t(b, co, h, w), dr.t(b, co, h, w, r=4)
        if dr.exact:
            y.view(-1)[0] = cs                               # planted: |y| == clamp is masked
            if y.numel() >= 2:
                y.view(-1)[-1] = -cs
        if case["mask_in_kernel"]:
            kw.update(g_rgb_small=gs, y_rgb_small=y, clamp_rgb_small=cs)
        else:
            kw.update(g_rgb_small=gs * (y.abs() < cs))       # masked by the caller
        kw.update(w_rgb_small=dr.t(co, c, r=2 if dr.exact else None), s_small=dr.t(b, c, r=2 if dr.exact else None))
    if case["g_direct"]:
        kw.update(g_direct=dr.t(b, h, w, c))
    if case["g_nchw3_a"]:
        kw.update(g_nchw3_a=dr.t(b, 3, h, w))
    if case["g_nchw3_b"]:
        kw.update(g_nchw3_b=dr.t(b, 3, h, w))
    q = 1.0
    if case["producer"]:
        p = dict(act=case["act"], alpha=dr.alpha, gain=dr.gain)
        if case["dcoef"]:
            p["dcoef"] = dr.dcoef(b, c)
        if case["bias"]:
            p["bias"] = dr.t(c)
        if case["noise"]:
            p["noise"] = dr.t(h, w)
            p["noise_strength"] = dr.strength
            if case["strength_dev"]:
                p["noise_strength_dev"] = torch.tensor(dr.strength)
                p["noise_strength"] = 8.0
        if case["clamp"]:
            p["clamp"] = clamp
        kw["producer"] = p
        # exact tier: g_pre is a multiple of alpha (gain >= 1), pre of 1/gain, noise * strength of `strength`, and 1/d and d of 1/2
        q = 0.25 * 0.5 * 0.5
    return kw, q


# ----------------------------------------------------------------------------- style_bwd cases
STYLE_CIN, STYLE_COUT = (3, 29, 32, 61, 512), (1, 63, 65, 512)


def style_cases(tier):
    """(Cin, Cout, w_dim, B, dd present, accumulate): every Cin in STYLE_CIN (both sides of the `i + 28 < Cin` unroll), every Cout
    in STYLE_COUT (around the 64-lane stride), w_dim 16 / 64 / 256 (80 in the realistic tier), B 1 and 3; the four combinations of
    dd present / absent and overwrite / accumulate at each Cin."""
    wdims = (16, 64, 256) + ((80,) if tier == "realistic" else ())
    cases = []
    for i, cin in enumerate(STYLE_CIN):
        for j in range(4):
            cases.append(dict(Cin=cin, Cout=STYLE_COUT[(i + j) % 4], w_dim=wdims[(i + j) % len(wdims)], B=(1, 3)[(i + j) % 2],
                              dd=j % 2 == 0, accumulate=j >= 2))
    return cases


def style_inputs(case, tier, seed=0):
    """fp32 CPU tensors of one affine layer's style gradient; exact tier: ranges shrink with Cin * Cout so that the sums stay below
    2^24 quanta; quantum: d^3 in eighths, style_gain 1/4, 1 / sqrt(w_dim) >= 1/16."""
    cin, cout, wd, b = case["Cin"], case["Cout"], case["w_dim"], case["B"]
    dr = Draw(tier, 7000 + 131 * cin + 17 * cout + wd + b + seed, r=1 if cin * cout > 4096 else (2 if cin * cout > 512 else 4))
    t = dict(ds=dr.t(b, cin), styles=dr.t(b, cin), affine_w=dr.t(cin, wd), dw0=dr.t(b, wd, r=4),
             style_gain=0.25 if dr.exact else f32(1.0 / math.sqrt(cin)))
    if case["dd"]:
        t.update(dd=dr.t(b, cout), dcoef=dr.dcoef(b, cout), wsq=dr.pos(cout, cin))
    else:
        t.update(dd=None, dcoef=None, wsq=None)
    return t, (0.125 * 0.25, 0.125 * 0.25 / math.sqrt(wd))          # quanta of dstot and of dw


def style_batch(layout, tier):
    """The item list of one ops.style_bwd_batch call: (dw0 [B,rows,w_dim], items, rows).  items: (tensors as style_inputs, case, ws
    row, reference dstot, its magnitude, quantum); rows: row -> (reference d_ws row, magnitude, N).  Layouts: 'one_launch' (12
    layers, three on each of four ws rows), 'two_launches' (34 layers, the cut after 32 falls between two rows), 'straddle' (34
    layers, row 16 would straddle the cut: the per-layer fallback)."""
    b, wd = 3, 80 if tier == "realistic" else 64
    n = 12 if layout == "one_launch" else 34
    row_of = {"one_launch": lambda i: (i * 5) % 4, "two_launches": lambda i: i // 2, "straddle": lambda i: (i + 1) // 2}[layout]
    nrows = max(row_of(i) for i in range(n)) + 2
    dw0 = Draw(tier, 31).t(b, nrows, wd)
    rows = {r: (dw0[:, r].double(), dw0[:, r].double().abs(), 16) for r in range(nrows)}
    items = []
    for i in range(n):
        cin, cout = STYLE_CIN[i % 5], STYLE_COUT[(i // 5 + i) % 4]
        case = dict(Cin=cin, Cout=cout, w_dim=wd, B=b, dd=i % 3 != 1)
        t, (q_s, _) = style_inputs(case, tier, seed=1000 * i)
        (r_s, r_w), (m_s, m_w) = style_bwd(t["ds"], t["dd"], t["styles"], t["dcoef"], t["wsq"], t["affine_w"], t["style_gain"])
        v, m, terms = rows[row_of(i)]
        rows[row_of(i)] = (v + r_w, m + m_w, terms + cin + cout + 32)
        items.append((t, case, row_of(i), r_s, m_s, q_s))
    return dw0, items, rows


# ----------------------------------------------------------------------------- conv_wgrad cases
WGRAD_SHAPES = (                      # (B, H, W, Cin, Cout), precisions, modes
    ((1, 4, 4, 8, 32), ("fp32",), ("3x3", "up", "1x1")),
    ((2, 9, 5, 24, 96), ("fp32",), ("3x3", "up", "1x1")),
    ((2, 5, 3, 64, 64), ("fp32", "bf16x3"), ("3x3", "up", "1x1")),
    ((1, 8, 9, 32, 128), ("fp32", "bf16x3"), ("up",)),
    # two samples, two position tiles each way with a ragged last row and column, two ci blocks (ci0 != 0 in the buffer resources
    # and in the slab epilogue)
    ((2, 5, 18, 128, 64), ("fp32", "bf16x3"), ("3x3", "up")),
    # Cin % 8 != 0: the per-element wgrad_reduce_kernel (the encoder's 4-channel input layer)
    ((1, 4, 4, 4, 32), ("fp32",), ("3x3", "up", "1x1")),
)


def wgrad_cases():
    return [(shape, prec, mode) for shape, precs, modes in WGRAD_SHAPES for prec in precs for mode in modes
            if not (prec == "bf16x3" and mode == "1x1")]                # (the 1x1 mode has no split-bf16 kernel)


def wgrad_split16(shape, prec, mode):
    """Whether the split-bf16 kernel takes the case (hfagp.h, HfagpWgradArgs::precision)."""
    _, _, _, cin, cout = shape
    return prec == "bf16x3" and mode in ("3x3", "up") and cout % 64 == 0 and (cin % 64 == 0 or (mode == "up" and cin == 32))


def wgrad_position_tiles(shape, prec, mode):
    """Position tiles of the kernel that runs: 2 x 16 positions (fp32 MFMA), 4 x 16 (split bf16)."""
    b, h, w, _, _ = shape
    rows = 4 if wgrad_split16(shape, prec, mode) else 2
    return b * (-(-h // rows)) * (-(-w // 16))


def wgrad_inputs(shape, mode, tier):
    """fp32 CPU tensors: x [B,H,W,Cin], styles, g_y (the gradient w.r.t. the layer's conv output: [B,H,W,Cout], or [B,2H,2W,Cout]
    before the FIR adjoint for 'up'), weight, sums [B,10,Cout] whose row 3 is dd, dcoef, dw0.  Quantum of the exact tier: d^3 in
    eighths; the FIR adjoint's taps in sixteenths."""
    b, h, w, cin, cout = shape
    dr = Draw(tier, 9000 + 7 * cin + cout + h + {"3x3": 0, "up": 1, "1x1": 2}[mode], r=2 if mode == "up" else 4)
    k = 1 if mode == "1x1" else 3
    up = 2 if mode == "up" else 1
    t = dict(x=dr.t(b, h, w, cin), styles=dr.t(b, cin), gy=dr.t(b, up * h, up * w, cout), weight=dr.t(cout, cin, k, k),
             sums=dr.t(b, 10, cout), dcoef=dr.dcoef(b, cout), dw0=dr.t(cout, cin, k, k, r=4))
    return t, 0.125 / (16.0 if mode == "up" else 1.0)


# ----------------------------------------------------------------------------- the smaller families
FIR_HW, FIR_C = ((1, 1), (3, 5), (8, 21)), (4, 12, 96)          # upfir_bwd / upsample2d_bwd: the exact tier only (dyadic taps)
AFFINE_CIN = (3, 32, 260, 512)
PLANES_CP = (4, 12, 32)


def affine_inputs(i, tier, ws):
    """Item i of an affine-gradient batch: (dstot [B,Cin], row view [B,w_dim] of ws [B,rows,w_dim], dA0, db0)."""
    b, rows, wd = ws.shape
    cin = AFFINE_CIN[i % 4]
    dr = Draw(tier, 11000 + i)
    return dr.t(b, cin), ws[:, i % rows], dr.t(cin, wd), dr.t(cin)

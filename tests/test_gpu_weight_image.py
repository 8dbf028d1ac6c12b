"""The 16-bit conv weight images (hfagp_weight_prep_prec / hfagp_weight_prep_batch) and every kernel that consumes one, at
weight scales from 2^-40 to 2^30.

a. every image against an independent torch-CPU rebuild of its contract, bit for bit (include/hfagp.h, "Weight images"):
   the bfloat16 kinds store successive round-to-nearest-even residuals of the weight itself; the float16 kinds store them of
   w * 2^-e, e the multiple of 8 that brings max |w| of the tensor into [2^-4, 2^4) (0 at unit scale: the image then has the raw
   weight's bits), and publish max |w| next to the image (`image.w_absmax`), from which every consumer recomputes e;
b. each consumer at weight = w0 * 2^k against a float64 reference of the same LINEAR operation: the bar of the precision class
   (SPLIT_TOL / F16_TOL of tests/test_gpu_parity.py, relative to max |ref|) is the same at every k, the output is finite, and
   y(w0 * 2^k) == 2^k * y(w0) bit for bit for the bfloat16 kinds and == 2^(k - k0) * y(w0 * 2^k0), k0 = k mod 8, for the float16 kinds
   (a power of two commutes with every rounding of the path; the float16 image's exponent moves in steps of 8);
c. one whole generator whose conv / toRGB weights carry per-layer factors 2^-12 ... 2^12, against the fp32 oracle.
Needs an MI355X:  python -m pytest tests -m gpu"""
import ctypes as C
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from hfa_gp_amd import _lib as L
from tests.test_gpu_parity import F16_TOL, SPLIT_TOL
from tests.util import make_inputs, state_cpu

pytestmark = pytest.mark.gpu

KINDS = ("bf16x3", "bf16x6", "f16", "f16x3")
TOL = dict(SPLIT_TOL, f16=F16_TOL)          # relative to max |ref|, at EVERY weight scale
KS = (-40, -20, -10, -7, -3, 0, 10, 13, 17, 30)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- a. the images, bit for bit
def _image_exponent(w):
    """e of the float16 kinds: max |w| = f 2^ex with f in [0.5, 1) -> e = 8 floor((ex + 3) / 8), the multiple of 8 that brings the
    maximum into [2^-4, 2^4) (0 for an all-zero or non-finite tensor)."""
    m = float(w.abs().max())
    if not (0.0 < m < 3.0e38):
        return 0
    return max(-120, min(120, 8 * math.floor((math.frexp(m)[1] + 3) / 8)))


def _rebuild(w, prec):
    """[parts, taps, Cin/8, Cout, 8] image of the fp32 weight w [Cout, Cin, k, k] on the CPU, and max |w| for the float16 kinds"""
    co, ci, kh, kw = w.shape
    absmax = None
    if prec in ("f16", "f16x3"):
        absmax = w.abs().max()
        w = w * 2.0 ** -_image_exponent(w)              # (a power of two as a Python float: exact, |e| <= 120)
        hi = w.half()
        parts = [hi] if prec == "f16" else [hi, (w - hi.float()).half()]
    else:
        parts, r = [], w.clone()
        for _ in range(2 if prec == "bf16x3" else 3):
            parts.append(r.bfloat16())
            r = r - parts[-1].float()
    img = torch.stack([p.reshape(co, ci // 8, 8, kh * kw).permute(3, 1, 0, 2) for p in parts]).contiguous()
    return img, absmax


def _edge_weight(cout, cin, k, seed):
    """N(0,1) weights with, on purpose: exact fp16 ties (both parities of the kept bit), values whose float16 residual is a
    subnormal, +-0, one tap plane at 2^-20 and one at 2^12 (k = 1: the two halves of the input channels instead)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g)
    flat = w.view(-1)
    n = flat[0::7].numel()            # ties: an odd 12-bit significand (the kept bit of either parity) times a power of two
    flat[0::7] = (2 * torch.randint(1024, 2048, (n,), generator=g) + 1).float() * 2.0 ** (torch.randint(-6, 3, (n,), generator=g).float() - 11)
    flat[1::7] *= -1.0
    flat[2::7] = 2.0 ** -4 * (1.0 + 2.0 ** -10 + 2.0 ** -21 + 2.0 ** -23)      # residual 2^-25 (1 + 2^-2): below fp16's normals
    flat[3::14] = 0.0
    flat[10::14] = -0.0
    if k == 3:
        w[:, :, 0, 1] *= 2.0 ** -20
        w[:, :, 2, 0] *= 2.0 ** 12
    else:
        w[:, : cin // 2] *= 2.0 ** -20
        w[:, cin // 2:] *= 2.0 ** 12
    return w


def _same_bits(img, want, absmax):
    got = img.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    have = getattr(img, "w_absmax", None)
    if absmax is None:
        assert have is None                       # bfloat16 has fp32's exponent range: the image is the weight itself
    else:
        assert have is not None, "a float16 image publishes max |w| of its tensor (hfagp.h)"
        assert torch.equal(have.cpu().view(torch.int32).reshape(()), absmax.view(torch.int32))


@pytest.mark.parametrize("prec", KINDS)
@pytest.mark.parametrize("cout,cin,k", [(128, 16, 3), (96, 32, 1), (32, 32, 3), (64, 96, 3), (40, 24, 3)])
def test_weight_prep_prec_is_the_contract_bit_for_bit(dev, cout, cin, k, prec):
    from hfa_gp_amd import ops
    w = _edge_weight(cout, cin, k, seed=cout + cin)
    _same_bits(ops.weight_prep_prec(w.to(dev), prec), *_rebuild(w, prec))
    _, wsq = ops.weight_prep(w.to(dev))
    assert torch.allclose(wsq.cpu().double(), (w.double() ** 2).sum((2, 3)), rtol=1e-6, atol=0)


@pytest.mark.parametrize("cout,cin,k", [(96, 32, 1), (32, 32, 3), (64, 96, 3)])
def test_weight_prep_batch_is_the_contract_bit_for_bit(dev, cout, cin, k):
    """forward image, image of the Cin/Cout transpose and wsq of several weights from one call; every kind on either side"""
    from hfa_gp_amd import ops
    w1, w2 = _edge_weight(cout, cin, k, seed=3), _edge_weight(cin, cout, k, seed=4) * 2.0 ** -9
    assert ops.weight_prep_batch_supported(w1)
    items = [(w1, "f16x3", "bf16x3", True), (w2, "bf16x6", "f16x3", True), (w1, "f16", "bf16x6", False), (w2, "bf16x3", "f16", True)]
    outs = ops.weight_prep_batch([(w.to(dev), p, pt, q) for w, p, pt, q in items])
    for (w, prec, prec_t, want_wsq), (img, img_t, wsq) in zip(items, outs):
        _same_bits(img, *_rebuild(w, prec))
        _same_bits(img_t, *_rebuild(w.transpose(0, 1).contiguous(), prec_t))
        if want_wsq:
            assert torch.allclose(wsq.cpu().double(), (w.double() ** 2).sum((2, 3)), rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------- b. every consumer, at every weight scale
def _inputs(b, h, w, cin, cout, taps, seed):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(b, cin, h, w, generator=g), "w": torch.randn(cout, cin, taps, taps, generator=g),
            "s": torch.randn(b, cin, generator=g) + 1.0, "d": torch.rand(b, cout, generator=g) + 0.5}


def _xs(t):
    return (t["x"] * t["s"][:, :, None, None]).double()


class Conv:
    """modconv in a fused-epilogue mode: styles and an explicit dcoef, nothing else (linear in the weight)"""
    taps, kinds, env = 3, KINDS, {}

    def __init__(self, b, h, w, cin, cout, mode="CONV3X3", ksplit=0, env=None, kinds=KINDS, split=False):
        self.shape, self.mode, self.ksplit, self.env, self.kinds, self.split = (b, h, w, cin, cout), mode, ksplit, env or {}, kinds, split
        self.taps = 1 if mode == "CONV1X1" else 3

    def inputs(self):
        return _inputs(*self.shape, self.taps, seed=sum(self.shape))

    def ref(self, t):
        return F.conv2d(_xs(t), t["w"].double(), padding=self.taps // 2) * t["d"].double()[:, :, None, None]

    def run(self, ops, t, wt):
        cout = self.shape[4]
        x = ops.nchw_to_nhwc(t["x"])
        if self.split:            # the route: K split through the workspace and the reducer
            a, *_ = ops._modconv_args(x, wt, cout, getattr(ops, self.mode), t["s"], t["d"], ksplit=self.ksplit)
            a.y = ops._NONNULL
            assert L.lib().hfagp_modconv_workspace_bytes(C.byref(a)) > 0
        return ops.nhwc_to_nchw(ops.modconv(x, wt, cout, getattr(ops, self.mode), styles=t["s"], dcoef=t["d"], ksplit=self.ksplit))


class Up2Raw(Conv):
    """CONVT3X3_UP2: the raw transposed conv (merged up-conv kernel); no epilogue, so no dcoef"""
    def __init__(self, b, h, w, cin, cout):
        super().__init__(b, h, w, cin, cout, mode="CONVT3X3_UP2")

    def ref(self, t):
        return F.conv_transpose2d(_xs(t), t["w"].transpose(0, 1).double(), stride=2)

    def run(self, ops, t, wt):
        return ops.nhwc_to_nchw(ops.modconv(ops.nchw_to_nhwc(t["x"]), wt, self.shape[4], ops.CONVT3X3_UP2, styles=t["s"]))


class UpconvFir(Conv):
    """upconv_fir (strip kernel, or the streaming Cin = 32 kernel when lean): transposed conv + FIR + dcoef, linear"""
    def __init__(self, b, h, w, cin, cout, lean):
        super().__init__(b, h, w, cin, cout, kinds=("bf16x3", "f16", "f16x3"),        # (images of one or two parts)
                         env={"HFAGP_DEV_FIR_MIN_BLOCKS": "1", "HFAGP_DEV_FIR_LEAN": "1" if lean else "0"})

    def ref(self, t):
        from oracle import eg3d_oracle as O
        return O._conv_up2(_xs(t), t["w"].double(), O.fir_kernel().double()) * t["d"].double()[:, :, None, None]

    def run(self, ops, t, wt):
        x, cout = ops.nchw_to_nhwc(t["x"]), self.shape[4]
        assert ops.upconv_fir_supported(x, wt, cout)
        return ops.nhwc_to_nchw(ops.upconv_fir(x, wt, cout, t["s"], t["d"], None, 0.0, None, act="linear", gain=1.0))


class TorgbSkip(Conv):
    """torgb_skip: the streaming 1x1 toRGB (no image to add, zero bias)"""
    def __init__(self, b, h, w, cin, cout):
        super().__init__(b, h, w, cin, cout, mode="CONV1X1")

    def ref(self, t):
        return F.conv2d(_xs(t), t["w"].double())

    def run(self, ops, t, wt):
        x, cout = ops.nchw_to_nhwc(t["x"]), self.shape[4]
        assert ops.torgb_skip_supported(x, wt, cout)
        return ops.nhwc_to_nchw(ops.torgb_skip(x, wt, cout, t["s"], torch.zeros(cout, device=x.device), None))


class BwdData(Conv):
    """CONV3X3_BWD / CONVS2_BWD on the image of the Cin/Cout TRANSPOSE (as weight_prep_batch emits it): gradient of the conv
    input, from a gradient g [B, Cout, ...]; no styles, no epilogue"""
    def __init__(self, b, h, cin, cout, up):
        super().__init__(b, h, h, cin, cout, mode="CONVS2_BWD" if up else "CONV3X3_BWD")
        self.taps, self.up = 3, up

    def inputs(self):
        b, h, _, cin, cout = self.shape
        g = torch.Generator().manual_seed(17 + h)
        ho = 2 * h + 1 if self.up else h
        return {"x": torch.randn(b, cout, ho, ho, generator=g), "w": torch.randn(cout, cin, 3, 3, generator=g)}

    def ref(self, t):
        if self.up:           # adjoint of conv_transpose2d(x, w^T, stride 2)
            return F.conv2d(t["x"].double(), t["w"].transpose(0, 1).double(), stride=2)
        return F.conv_transpose2d(t["x"].double(), t["w"].double(), padding=1)

    transposed = True

    def run(self, ops, t, wt):
        b, h, _, cin, cout = self.shape
        g = ops.nchw_to_nhwc(t["x"])
        if self.up:           # the four parity images of the gradient of y_t: [a][b][B][H+1][W+1][Cout], zero past the odd extents
            par = torch.zeros(2, 2, b, h + 1, h + 1, cout, device=g.device)
            for a in range(2):
                for c in range(2):
                    par[a, c, :, : h + 1 - a, : h + 1 - c] = g[:, a::2, c::2]
            g = par
        return ops.nhwc_to_nchw(ops.modconv(g, wt, cin, getattr(ops, self.mode)))


CONSUMERS = {
    "staged16": Conv(2, 40, 40, 16, 128),                                                  # staged 3x3, 16-channel loop
    # (ksplit=1: the epilogue in the conv kernel; the plan's own choice at this size is two K slices, "splitk3" covers the reducer)
    "staged16_cin64": Conv(2, 40, 40, 64, 128, ksplit=1, env={"HFAGP_DEV_CONV9_LEGACY": "1"}),   # the same loop at a conv9 shape
    "conv9_32": Conv(2, 40, 40, 64, 128, ksplit=1, kinds=("f16x3",)),                      # 32-channel 16x16x32 loop
    "splitk3": Conv(2, 40, 40, 64, 128, ksplit=3, split=True),                             # K split by force (f16x3: the 32-channel loop)
    "small": Conv(2, 5, 7, 64, 96),                                                        # csrc/smallconv.hip (<= 256 positions)
    "conv1x1_96": Conv(2, 19, 19, 32, 96, mode="CONV1X1", ksplit=1),                       # staged 1x1 on the padded 128-wide tile
    "up2_raw": Up2Raw(1, 9, 9, 16, 128),
    "upconv_fir": UpconvFir(2, 24, 40, 32, 128, lean=False),
    "upconv_fir_lean": UpconvFir(2, 24, 40, 32, 128, lean=True),
    "torgb_skip": TorgbSkip(1, 128, 128, 16, 96),
    "conv3x3_bwd": BwdData(2, 17, 128, 32, up=False),
    "convs2_bwd": BwdData(2, 7, 128, 16, up=True),
}
_CASES = [(name, prec) for name, c in CONSUMERS.items() for prec in c.kinds]
_STATE = {}           # consumer -> (device inputs, float64 reference at k = 0); (consumer, kind) -> output at k = 0


def _setup(name, dev):
    if name not in _STATE:
        c = CONSUMERS[name]
        t = c.inputs()
        _STATE[name] = ({k: v.to(dev) for k, v in t.items()}, c.ref(t))
    return _STATE[name]


def _consume(name, prec, k, dev, monkeypatch):
    from hfa_gp_amd import ops
    c = CONSUMERS[name]
    for var in ("HFAGP_DEV_CONV9_LEGACY", "HFAGP_DEV_FIR_MIN_BLOCKS", "HFAGP_DEV_FIR_LEAN", "HFAGP_DEV_FIR_NSEG"):
        monkeypatch.delenv(var, raising=False)
    for var, val in c.env.items():
        monkeypatch.setenv(var, val)
    t, ref0 = _setup(name, dev)
    w = t["w"] * 2.0 ** k             # exact: |w0| 2^k stays among fp32's normals (a float factor: pow() on the device is not exact)
    if getattr(c, "transposed", False):
        w = w.transpose(0, 1).contiguous()
    y = c.run(ops, t, ops.weight_prep_prec(w, prec)).cpu()
    return y, ref0 * 2.0 ** k                   # the operation is linear in w: ref(w0 2^k) = 2^k ref(w0), exactly


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,prec", _CASES)
def test_consumer_holds_its_class_at_every_weight_scale(dev, monkeypatch, name, prec, k):
    y, ref = _consume(name, prec, k, dev, monkeypatch)
    assert y.shape == ref.shape
    finite = bool(torch.isfinite(y).all())
    err, top = float((y.double() - ref).abs().max()), float(ref.abs().max())
    print(f"{name} {prec} k={k}: finite {finite}, max err {err:.3e} = {err / top:.3e} of max |ref| (bar {TOL[prec]:.1e})")
    assert finite
    assert err <= TOL[prec] * top, (err / top, TOL[prec])
    # the bfloat16 image is the weight: y(w0 2^k) = 2^k y(w0).  The float16 image's exponent moves in steps of 8, so the identity
    # holds from the k of the same residue: y(w0 2^k) = 2^(k - k0) y(w0 2^k0), k0 = k mod 8
    k0 = k % 8 if prec in ("f16", "f16x3") else 0
    if (name, prec, k0) not in _STATE:
        _STATE[(name, prec, k0)] = y if k == k0 else _consume(name, prec, k0, dev, monkeypatch)[0]
    assert torch.equal(y, _STATE[(name, prec, k0)] * 2.0 ** (k - k0)), f"y(w0 2^{k}) != 2^{k - k0} y(w0 2^{k0})"


def test_conv9_32_channel_loop_is_the_route_taken(dev, monkeypatch):
    """(the 32- and the 16-channel loop sum in different orders: equal bits would mean the developer switch did nothing)"""
    new, _ = _consume("conv9_32", "f16x3", 0, dev, monkeypatch)
    old, _ = _consume("staged16_cin64", "f16x3", 0, dev, monkeypatch)
    assert not torch.equal(new, old)


@pytest.mark.parametrize("k", KS)
def test_f16_storage_conv_at_every_weight_scale(dev, k):
    """fp16 STORAGE (float16 x, y_f16) on the single-pass fp16 image.  A float16 OUTPUT cannot follow the weight's scale, so the
    explicit dcoef carries 2^-k, as the demodulation of such a weight would: the result is then the same, bit for bit, at every k of one residue mod 8
    (the step of the image's exponent).
    Bounds: the storage path's own (tests/test_gpu_round2.py: 2e-3 of the scale against the fp32-stored run of the same image) and
    F16_TOL against float64."""
    from hfa_gp_amd import ops
    b, h, cin, cout = 2, 40, 16, 128
    assert ops.f16_storage_supported(h, h, cin, cout, b)
    if "f16io" not in _STATE:
        t = _inputs(b, h, h, cin, cout, 3, seed=77)
        xh = t["x"].half()
        ref = F.conv2d((xh.double() * t["s"].double()[:, :, None, None]), t["w"].double(), padding=1) * t["d"].double()[:, :, None, None]
        _STATE["f16io"] = ({n: v.to(dev) for n, v in t.items()}, ref, {})
    t, ref, seen = _STATE["f16io"]
    wt = ops.weight_prep_prec(t["w"] * 2.0 ** k, "f16")
    d = t["d"] * 2.0 ** -k
    xh = ops.nchw_to_nhwc(t["x"]).half()
    y = ops.modconv(xh, wt, cout, ops.CONV3X3, styles=t["s"], dcoef=d, y_f16=True)
    y32 = ops.modconv(xh.float(), wt, cout, ops.CONV3X3, styles=t["s"], dcoef=d)
    assert y.dtype == torch.float16 and torch.isfinite(y).all() and torch.isfinite(y32).all()
    scale = float(y32.abs().max())
    err = float((y.float() - y32).abs().max())
    err64 = float((ops.nhwc_to_nchw(y.float()).cpu().double() - ref).abs().max())
    print(f"f16 storage k={k}: {err / scale:.3e} of the scale against fp32 storage, {err64 / float(ref.abs().max()):.3e} against float64")
    assert err <= 2e-3 * scale
    assert err64 <= F16_TOL * float(ref.abs().max())
    seen.setdefault(k % 8, y)
    assert torch.equal(y, seen[k % 8])


# ----------------------------------------------------------------------------- c. a whole generator
def test_generator_with_per_layer_power_of_two_weight_scales(dev):
    """tests/test_gpu_round3.py::test_trained_weight_statistics_stress with every conv / toRGB weight times a per-layer 2^k,
    k from {-12 ... 12} (demodulation makes the scale of a conv weight free, so a checkpoint may put a layer anywhere): same
    assertions — planes within 5e-5 max(1, |planes|) of the fp32 oracle, the image against the exact-fp32 generator's own distance."""
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = PRESETS["small128"]()
    assert cfg.conv_precision == "f16x3"
    gen = TriPlaneGenerator(cfg, seed=5)
    g = torch.Generator().manual_seed(29)
    ks = []
    with torch.no_grad():
        for name, p in gen.named_parameters():
            if name.startswith("backbone.mapping."):
                continue
            if name.endswith(".weight") and ".affine." not in name and p.dim() == 4:
                ks.append(int(torch.randint(-12, 13, (), generator=g)))
                p.mul_(2.0 ** ks[-1])
    assert min(ks) <= -8 and max(ks) >= 8, ks
    P = state_cpu(gen)
    exact = TriPlaneGenerator(dataclasses.replace(cfg, conv_precision="fp32", decoder_precision="fp32"), seed=5)
    exact.load_state_dict(gen.state_dict())
    gen, exact = gen.to(dev), exact.to(dev)
    ws, c, us, ui = make_inputs(cfg, 1, seed=21)
    ref = O.synthesis(P, cfg, ws, c, us, ui, return_planes=True)
    pr = cfg.plane_resolution
    pmax, imax = float(ref["planes"].abs().max()), float(ref["image"].abs().max())
    err = {}
    for tag, g_ in (("f16x3", gen), ("exact_fp32", exact)):
        out = g_.synthesis(ws.to(dev), c.to(dev), noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), return_planes=True)
        assert torch.isfinite(out["image"]).all()
        planes = out["planes"].permute(0, 1, 4, 2, 3).reshape(1, 96, pr, pr).cpu()
        err[tag] = {"planes": float((planes - ref["planes"]).abs().max()),
                    "image_raw": float((out["image_raw"].cpu() - ref["image_raw"]).abs().max()),
                    "image": float((out["image"].cpu() - ref["image"]).abs().max())}
    print(f"per-layer 2^k, k = {ks}: |planes| max {pmax:.3g}, |image| max {imax:.3g}; max abs error vs the oracle {err}")
    assert err["f16x3"]["planes"] <= 5e-5 * max(1.0, pmax), (err, pmax)
    for key in ("image_raw", "image"):
        floor = 1e-4 * max(1.0, imax if key == "image" else 1.0)
        assert err["f16x3"][key] <= max(2.0 * err["exact_fp32"][key], floor), (key, err)

"""The forward streaming kernels (csrc/elementwise.hip) against the float64 reference of tests/forward_ref.py, one entry point at
a time, in two tiers:

  exact      integer inputs and power-of-two scalars: bit for bit (indexing, borders, strips, variant dispatch, tails; no
             tolerance); every case asserts its precondition (backward_ref.exact_precondition; fp16 storage: the stored value is a
             multiple of the quantum below 2^11 quanta), which tests/test_forward_ref_cpu.py also runs without a GPU.
  realistic  randn inputs: |got - ref| <= (N + 16) 2^-24 magnitude for every element, N = the number of terms summed into it
             (written next to each `hold`).  fp16 storage: the reference reads the stored halves as they are, and the bar grows by
             2^-11 |ref| for the final rounding (every reference value is asserted to be a normal fp16 number).  The bound is
             derived (backward_ref.bound), never measured; the worst error / bound per family is printed and recorded in
             profiles/forward_kernels_f64.md.

lrelu and clamp are continuous with slope at most `gain`: the bound passes through them scaled by `gain`, and no element is
excluded.  dcoef = rsqrt(sum of NON-NEGATIVE terms + eps): the sum's relative error is at most (Cin + 3) u, the inverse square root
halves it, and the 16 units of slack cover the rsqrt instruction's own error; its reference takes the kernel's styles as given.
dcoef is held to that bar in both tiers (the instruction is not exact arithmetic).

Needs an MI355X:  python -m pytest tests/test_gpu_forward_kernels.py -m gpu"""
import math

import pytest
import torch

from tests import forward_ref as R

pytestmark = pytest.mark.gpu

TIERS = R.TIERS
WORST = {}                     # family -> largest error / bound seen in the realistic tier


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for family in sorted(WORST):
        print(f"\nworst error / bound [{family}]: {WORST[family]:.4f}", end="")


def to_dev(v, dev):
    return v.to(dev) if torch.is_tensor(v) else v


def hold(tier, family, got, ref, mag, n, what, half=False):
    """Exact tier: bit for bit.  Realistic tier: every element within (n + 16) u of its magnitude (+ 2^-11 |ref| in fp16 storage)."""
    assert got.shape == ref.shape and got.dtype == (torch.float16 if half else torch.float32), what
    if tier == "exact":
        bad = (got.double().cpu() != ref).sum().item()
        assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the float64 reference"
        return
    ratio = (R.worst_ratio_f16 if half else R.worst_ratio)(got, ref, mag, n)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    assert ratio <= 1.0, f"{family} {what}: error is {ratio:.3f} of the bound (N = {n})"


def f16_up(v):
    """The upper fp16 neighbour of a non-negative normal fp16 number."""
    return v + 2.0 ** (math.frexp(v)[1] - 11) if v > 0 else 2.0 ** -24


def hold_absmax(run, got, half, what):
    """`run(slots)` launches with the given slot buffer.  On a zeroed buffer the maximum over the slots is max |y| of the returned
    tensor (fp16 storage: between max |stored y| and its upper fp16 neighbour); a buffer holding a larger value keeps it."""
    slots = torch.zeros(R.ABSMAX_SLOTS * R.ABSMAX_STRIDE, device=got.device)
    again = run(slots)
    assert torch.equal(again, got), what
    top, ymax = R.absmax_of(slots), got.float().abs().max().item()
    if half:
        assert ymax <= top <= f16_up(ymax), f"{what}: published {top!r}, max |stored y| {ymax!r}"
    else:
        assert top == ymax, f"{what}: published {top!r}, max |y| {ymax!r}"
    big = 2.0 * ymax + 1.0
    slots.fill_(big)
    run(slots)
    assert (slots == big).all(), f"{what}: a slot holding a larger value was overwritten"


# ----------------------------------------------------------------------------- hfagp_upfir_epilogue_fwd
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("h,w", R.UPFIR_HW)
@pytest.mark.parametrize("c", R.UPFIR_C)
def test_upfir_epilogue(dev, c, h, w, storage, tier):
    """FIR + epilogue at one output pixel pair (every tap row and column on a border), exactly one strip, a strip plus a ragged
    tail and a wide image; B 1 and 2; dcoef, noise and bias each present and absent; both activations; clamp on and off; planted
    pre-activation values 0 and +-clamp / gain; y_absmax from launches with a partial wave and (C 64) with full waves only."""
    from hfa_gp_amd import ops
    half = storage == "fp16"
    for case in R.upfir_cases(c, (h, w), half, tier):
        kw, q = R.upfir_inputs(case)
        ref, mag = R.upfir_epilogue(**kw)
        what = "B{B} dcoef={dcoef} noise={noise} bias={bias} {act} clamp={clamp}".format(**case)
        if tier == "exact":
            (R.f16_precondition if half else R.exact_precondition)(ref, mag, q, what)
            R.upfir_planted(case, ref)
        elif half:
            R.f16_in_normal_range(ref, what)
        d = {k: to_dev(v, dev) for k, v in kw.items()}

        def run(slots):
            return ops.upfir_epilogue(d["yt"], d.get("dcoef"), d.get("noise"), d["strength"], d.get("bias"), d["act"], d["alpha"],
                                      d["gain"], d["clamp"], y_absmax=slots)
        got = run(None)
        hold(tier, f"upfir_epilogue {storage}", got, ref, mag, R.UPFIR_N, what, half)          # N = 16 taps + 3 (dcoef, noise, bias)
        if case["dcoef"] == case["noise"] == case["bias"]:                                      # all operands / none: 16 launches
            hold_absmax(run, got, half, what)


# ----------------------------------------------------------------------------- hfagp_skip_upsample_add
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("img", R.SKIP_IMG, ids=lambda v: "none" if v is None else f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("c", R.SKIP_C)
def test_skip_upsample_add(dev, c, img, tier):
    """upsample2d(img) + y at one image pixel (all four taps of every output pixel touch a border), ragged sizes and without an
    image; plain and plane-major stores (C 12: one float4 per plane; C 96: 32 channels per plane); out_absmax."""
    from hfa_gp_amd import ops
    for b in R.SKIP_B:
        im, y, q = R.skip_inputs(c, img, b, tier)
        im_d, y_d = to_dev(im, dev), y.to(dev)
        for plane_major in ((False, True) if c % 12 == 0 else (False,)):
            ref, mag = R.skip_upsample_add(im, y, plane_major)
            what = f"B{b} plane_major={plane_major}"
            if tier == "exact":
                R.exact_precondition(ref, mag, q, what)

            def run(slots):
                return ops.skip_upsample_add(im_d, y_d, plane_major=plane_major, out_absmax=slots)
            got = run(None)
            hold(tier, "skip_upsample_add", got, ref, mag, R.SKIP_N, what)                      # N = 4 taps + y
            hold_absmax(run, got, False, what)


# ----------------------------------------------------------------------------- hfagp_torgb_fwd, hfagp_torgb_finish_fwd
def _torgb_run(fn, first, t, flags, hw, b, cout, clamp, dev):
    rgb_in, clamp_on, pre_on = flags
    y_pre = torch.full((b, cout, hw[0], hw[1]), -7.0, device=dev) if pre_on else None
    out = fn(*first, t["bias"], t["rgb_in"] if rgb_in else None, clamp if clamp_on else None, y_pre)
    return out, y_pre


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("cout", R.TORGB_COUT)
@pytest.mark.parametrize("cin", R.TORGB_CIN_LDS + R.TORGB_CIN_REG)
def test_torgb_small(dev, cin, cout, tier):
    """The LDS kernel (Cin 8, 24, 512) and the six register kernels (Cin 64 / 128 / 256, three or four accumulators) at 1 .. 4
    output channels; 4 pixels (fewer than one 32-pixel row of a block), 60, and 288 (one full 256-pixel block of the register
    kernels and a partial one); rgb_in, clamp and y_pre each present and absent; y_pre is the value before the clamp."""
    from hfa_gp_amd import ops
    clamp = R.torgb_clamp(cin, tier)
    for hw in R.TORGB_HW:
        for b in (1, 2):
            t, q = R.torgb_inputs(cin, cout, hw, b, tier)
            d = {k: v.to(dev) for k, v in t.items()}
            for flags in R.TORGB_FLAGS:
                (r_out, r_pre), (m_out, m_pre) = R.torgb_small(t["x"], t["weight"], t["styles"], t["bias"], t["rgb_in"] if flags[0] else None,
                                                               clamp if flags[1] else None)
                what = f"{hw[0]}x{hw[1]} B{b} rgb_in={flags[0]} clamp={flags[1]}"
                if tier == "exact":
                    R.exact_precondition(r_out, m_out, q, what)
                    R.exact_precondition(r_pre, m_pre, q, what)
                out, y_pre = _torgb_run(ops.torgb_small, (d["x"], d["weight"], d["styles"]), d, flags, hw, b, cout, clamp, dev)
                kind = "reg" if cin in R.TORGB_CIN_REG else "lds"
                hold(tier, f"torgb_small {kind}", out, r_out, m_out, cin + 5, what)            # N = Cin + bias + 4 skip taps
                if y_pre is not None:
                    hold(tier, f"torgb_small {kind} y_pre", y_pre, r_pre, m_pre, cin + 1, what + " y_pre")      # N = Cin + bias


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("cout", R.FINISH_COUT)
@pytest.mark.parametrize("nparts", R.FINISH_NPARTS)
def test_torgb_finish(dev, nparts, cout, tier):
    """Sum of the partial images (their fourth channel is not read), bias, y_pre, clamp, skip."""
    from hfa_gp_amd import ops
    for hw in R.TORGB_HW:
        for b in (1, 2):
            t, q = R.finish_inputs(nparts, cout, hw, b, tier)
            t["part"][..., 3] = 1000.0
            d = {k: v.to(dev) for k, v in t.items()}
            for flags in R.TORGB_FLAGS:
                (r_out, r_pre), (m_out, m_pre) = R.torgb_finish(t["part"], t["bias"], t["rgb_in"] if flags[0] else None,
                                                                R.CLAMP[tier] if flags[1] else None)
                what = f"{hw[0]}x{hw[1]} B{b} rgb_in={flags[0]} clamp={flags[1]}"
                if tier == "exact":
                    R.exact_precondition(r_out, m_out, q, what)
                out, y_pre = _torgb_run(ops.torgb_finish, (d["part"],), d, flags, hw, b, cout, R.CLAMP[tier], dev)
                hold(tier, "torgb_finish", out, r_out, m_out, nparts + 5, what)                 # N = nparts + bias + 4 skip taps
                if y_pre is not None:
                    hold(tier, "torgb_finish y_pre", y_pre, r_pre, m_pre, nparts + 1, what + " y_pre")


# ----------------------------------------------------------------------------- hfagp_style_fwd, hfagp_style_batch_fwd
def _hold_styles(tier, family, t, q, styles, dcoef, what):
    (r_s, _), (m_s, _) = R.styles_demod(t["ws"][:, 1], t["affine_w"], t["affine_b"], None, t["style_gain"], t["eps"])
    wd, cin = t["affine_w"].shape[1], t["affine_w"].shape[0]
    if tier == "exact":
        R.exact_precondition(r_s, m_s, q, what)
    hold(tier, f"{family} styles", styles, r_s, m_s, wd + 1, what)                              # N = w_dim + bias
    assert (dcoef is None) == (t["wsq"] is None), what
    if dcoef is not None:
        r_d, m_d = R.demod(styles.cpu(), t["wsq"], t["eps"])                                    # (the kernel's own styles, as given)
        hold("realistic", f"{family} dcoef", dcoef, r_d, m_d, cin, what + " dcoef")             # N = Cin (module docstring)


@pytest.mark.parametrize("cin", R.STYLE_CIN)
@pytest.mark.parametrize("wd,tier", R.STYLE_PARAMS)
def test_styles_demod(dev, wd, cin, tier):
    """w_dim 4, 64, 260 (one full 256-wide trip of the wave and a tail), 512; Cin and Cout around the 64-lane stride; B 1 and 3; w
    contiguous and as the strided row view ws[:, 1] of [B, 3, w_dim]; with and without wsq.  Exact tier: w_dim 4 and 64 only, where
    1 / sqrt(w_dim) is a power of two."""
    from hfa_gp_amd import ops
    for cout in R.STYLE_COUT:
        for b in R.STYLE_B:
            t, q = R.style_inputs(wd, cin, cout, b, tier)
            d = {k: to_dev(v, dev) for k, v in t.items()}
            for strided in (False, True):
                w = d["ws"][:, 1] if strided else d["ws"][:, 1].contiguous()
                assert w.is_contiguous() == (not strided or b == 1)
                styles, dcoef = ops.styles_demod(w, d["affine_w"], d["affine_b"], d["wsq"], t["style_gain"], t["eps"])
                _hold_styles(tier, "styles_demod", t, q, styles, dcoef, f"Cout {cout} B{b} strided={strided}")


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n", [1, 3, 32])
def test_styles_demod_batch(dev, n, tier):
    """One launch for layers of different B * Cin and B * Cout (the grid of the largest overhangs the others), items without dcoef
    between items with; every output against the reference, and — at w_dim 64, 260, 512 — bit for bit what ops.styles_demod gives
    for the same item: the two kernels form the 1 / sqrt(w_dim) gain the same way."""
    from hfa_gp_amd import ops
    ref_items = R.style_batch_items(n, tier)
    items, dev_items = [], []
    for _, (t, _) in ref_items:
        d = {k: to_dev(v, dev) for k, v in t.items()}
        dev_items.append(d)
        items.append((d["ws"][:, 1], d["affine_w"], d["affine_b"], d["wsq"], t["style_gain"], t["eps"]))
    outs = ops.styles_demod_batch(items)
    assert len(outs) == n
    for i, ((wd, (t, q)), item, (styles, dcoef)) in enumerate(zip(ref_items, items, outs)):
        _hold_styles(tier, "styles_demod_batch", t, q, styles, dcoef, f"item {i}")
        if wd in (64, 260, 512):
            s1, d1 = ops.styles_demod(*item)
            assert torch.equal(styles, s1), f"item {i} (w_dim {wd}): styles differ from ops.styles_demod by {(styles - s1).abs().max().item():.3e}"
            assert (dcoef is None and d1 is None) or torch.equal(dcoef, d1), f"item {i}: dcoef differs from ops.styles_demod"


# ----------------------------------------------------------------------------- hfagp_fc_fwd, hfagp_weight_prep
@pytest.mark.parametrize("fin,tier", R.FC_PARAMS)
def test_fully_connected(dev, fin, tier):
    """In around the 64-lane stride and at 512; Out 1 and 5; B 1 and 3; with and without bias; both activations; lr_mul 0.5 (exact
    tier: In 1 and 64, where lr_mul / sqrt(In) is a power of two) and 0.01."""
    from hfa_gp_amd import ops
    for fout, b, bias, act in R.fc_cases():
        t, q = R.fc_inputs(fin, fout, b, tier)
        bs = t["bias"] if bias else None
        ref, mag = R.fully_connected(t["x"], t["weight"], bs, t["lr_mul"], act, t["alpha"], t["gain"])
        what = f"Out {fout} B{b} bias={bias} {act}"
        if tier == "exact":
            R.exact_precondition(ref, mag, q, what)
        got = ops.fully_connected(t["x"].to(dev), t["weight"].to(dev), to_dev(bs, dev), t["lr_mul"], act, t["alpha"], t["gain"])
        hold(tier, "fully_connected", got, ref, mag, fin + 1, what)                             # N = In + bias


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("co,ci,k", R.WPREP)
def test_weight_prep(dev, co, ci, k, tier):
    """The fp32 weight image is a permutation (bit for bit in both tiers); wsq = sum over the taps of w^2."""
    from hfa_gp_amd import ops
    wt = R.Draw(tier, co).t(co, ci, k, k)
    (r_img, r_sq), (_, m_sq) = R.weight_prep(wt)
    if tier == "exact":
        R.exact_precondition(r_sq, m_sq, 1.0, "wsq")
    img, wsq = ops.weight_prep(wt.to(dev))
    hold("exact", "", img, r_img, r_img.abs(), 1, "wt")
    hold(tier, "weight_prep wsq", wsq, r_sq, m_sq, k * k, "wsq")                                # N = taps


# ----------------------------------------------------------------------------- blur, upfirdn2d, bias_act, layouts
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("c", R.BLUR_C)
@pytest.mark.parametrize("h,w", R.BLUR_HW)
def test_blur_down_and_its_adjoint(dev, h, w, c, tier):
    """One output pixel (every tap row and column on a border) and ragged sizes; the adjoint through autograd of ops.blur_down."""
    from hfa_gp_amd import ops
    for b in R.BLUR_B:
        dr = R.Draw(tier, 100 * h + 10 * w + c + b)
        x, gy = dr.t(b, h, w, c), dr.t(b, h // 2, w // 2, c)
        (ref, mag), (gref, gmag) = R.blur_down(x), R.blur_down_bwd(gy)
        if tier == "exact":
            R.exact_precondition(ref, mag, 1 / 64, "blur_down")
            R.exact_precondition(gref, gmag, 1 / 64, "blur_down_bwd")
        x_d = x.to(dev).requires_grad_(True)
        y = ops.blur_down(x_d)
        y.backward(gy.to(dev))
        hold(tier, "blur_down", y.detach(), ref, mag, 16, f"B{b}")                              # N = 16 taps
        hold(tier, "blur_down_bwd", x_d.grad, gref, gmag, 16, f"B{b} adjoint")                  # N <= 16 taps (4 per pixel)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("up,down,pad", R.UPFIRDN)
def test_upfirdn2d_forward(dev, up, down, pad, tier):
    """A 3 x 4 filter that is neither square nor symmetric: a flip or a transposition of the taps shows."""
    from hfa_gp_amd import ops
    x, q = R.upfirdn_inputs(up, down, tier)
    f = R.upfirdn_filter()
    ref, mag = R.upfirdn2d(x, f, up, down, pad, float(up * up))
    if tier == "exact":
        R.exact_precondition(ref, mag, q, "upfirdn2d")
    got = ops.upfirdn2d(x.to(dev), f.to(dev), up=up, down=down, padding=pad, gain=float(up * up))
    hold(tier, "upfirdn2d", got, ref, mag, 12, "upfirdn2d")                                     # N = fh * fw = 3 * 4


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("shape,dim", [((2, 3, 5, 7), 1), ((2, 5, 7, 8), 3), ((2, 3, 1024, 400), 1)], ids=["dim1", "dim3", "two-trips"])
def test_bias_act_forward(dev, shape, dim, tier):
    """Bias along dim 1 and along the last dim; 2 457 600 elements (more than 8192 blocks of 256: the grid-stride loop takes a second
    trip); planted pre-activation values 0 and +-clamp / gain."""
    from hfa_gp_amd import ops
    big = math.prod(shape) > 8192 * 256
    assert big == (shape[2] == 1024)
    x, b, dr, q = R.bias_act_inputs(shape, dim, tier)
    x_d, b_d = x.to(dev), b.to(dev)
    for act, clamp, bias in ((("lrelu", R.CLAMP[tier], True),) if big else
                             [(a, cl, bs) for a in ("linear", "lrelu") for cl in (None, R.CLAMP[tier]) for bs in (True, False)]):
        ref, mag = R.bias_act(x, b if bias else None, dim, act, dr.alpha, dr.gain, clamp)
        if tier == "exact":
            R.exact_precondition(ref, mag, q, "bias_act")
        got = ops.bias_act(x_d, b_d if bias else None, dim, act, dr.alpha, dr.gain, clamp)
        hold(tier, "bias_act", got, ref, mag, 2, f"{act} clamp={clamp} bias={bias}")            # N = x + bias


@pytest.mark.parametrize("c,hw", R.TRANSPOSE)
def test_layout_transposes_are_permutations(dev, c, hw):
    """Channel counts and pixel counts on both sides of the 32 x 32 tile; H * W = 1."""
    from hfa_gp_amd import ops
    for b in (1, 2):
        x = torch.randn(b, c, hw, 1, generator=torch.Generator().manual_seed(c + hw + b))
        got = ops.nchw_to_nhwc(x.to(dev))
        assert torch.equal(got.cpu().double(), R.nchw_to_nhwc(x)[0])
        assert torch.equal(ops.nhwc_to_nchw(got).cpu().double(), R.nhwc_to_nchw(got.cpu())[0]) and torch.equal(ops.nhwc_to_nchw(got).cpu(), x)


# ----------------------------------------------------------------------------- documented refusals
def test_documented_refusals_raise_and_launch_nothing(dev):
    """A mis-shaped operand of the streaming wrappers (every extent the kernels would otherwise read or write past), and what the
    library refuses (C % 4 != 0, plane-major C no multiple of 12, five toRGB channels, odd toRGB H or W, w_dim % 4 != 0, 33 batch
    items): a Python exception each, the output-side tensors untouched, the device still healthy."""
    from hfa_gp_amd import ops
    z = lambda *s: torch.ones(*s, device=dev)        # noqa: E731
    slots, short = z(R.ABSMAX_SLOTS * R.ABSMAX_STRIDE), z(64)
    cases = []

    def refuses(match, fn, *args, **kw):
        cases.append(match)
        with pytest.raises(RuntimeError, match=match):
            fn(*args, **kw)

    # upfir_epilogue
    for shape in ((1, 4, 5, 4), (1, 5, 4, 4), (1, 1, 5, 4), (1, 5, 1, 4), (1, 6, 6, 4)):
        refuses("yt must be", ops.upfir_epilogue, z(*shape), None, None, 0.0, None, y_absmax=slots)
    yt = z(2, 5, 5, 8)
    for dcoef in (z(1, 8), z(2, 4), z(2, 16)[:, ::2], torch.ones(2, 8), z(2, 8).half()):
        refuses("dcoef must be", ops.upfir_epilogue, yt, dcoef, None, 0.0, None, y_absmax=slots)
    for noise in (z(4, 3), z(3, 4), z(16), z(4, 4).double()):
        refuses("noise must be", ops.upfir_epilogue, yt, None, noise, 0.5, None, y_absmax=slots)
    for bias in (z(4), z(1, 8), z(7)):
        refuses("bias must be", ops.upfir_epilogue, yt, None, None, 0.0, bias, y_absmax=slots)
    refuses("y_absmax must be", ops.upfir_epilogue, yt, None, None, 0.0, None, y_absmax=short)
    refuses("multiple of 4", ops.upfir_epilogue, z(1, 5, 5, 6), None, None, 0.0, None, y_absmax=slots)
    # skip_upsample_add
    y = z(2, 4, 6, 12)
    for img in (z(2, 2, 2, 12), z(2, 3, 3, 12), z(1, 2, 3, 12), z(2, 2, 3, 8), z(2, 4, 6, 12)):
        refuses("img must be", ops.skip_upsample_add, img, y, out_absmax=slots)
    refuses("even height and width", ops.skip_upsample_add, z(2, 1, 3, 12), z(2, 3, 6, 12), out_absmax=slots)
    refuses("out_absmax must be", ops.skip_upsample_add, None, y, out_absmax=short)
    refuses("unsupported channel count", ops.skip_upsample_add, z(1, 2, 2, 6), z(1, 4, 4, 6), out_absmax=slots)
    refuses("unsupported channel count", ops.skip_upsample_add, z(1, 2, 2, 8), z(1, 4, 4, 8), plane_major=True, out_absmax=slots)
    # torgb_small
    x, wt, st, bs = z(2, 4, 6, 8), z(3, 8), z(2, 8), z(3)
    y_pre = z(2, 3, 4, 6)
    refuses("weight must be", ops.torgb_small, x, z(3, 4), st, bs, None, None, y_pre)
    refuses(r"weight \[Cout, Cin\]", ops.torgb_small, x, z(3, 8, 1, 1), st, bs, None, None, y_pre)
    for styles in (z(2, 4), z(1, 8), z(2, 16)):
        refuses("styles must be", ops.torgb_small, x, wt, styles, bs, None, None, y_pre)
    refuses("bias must be", ops.torgb_small, x, wt, st, z(2), None, None, y_pre)
    for rgb_in in (z(2, 3, 2, 2), z(2, 3, 4, 6), z(1, 3, 2, 3), z(2, 2, 2, 3)):
        refuses("rgb_in must be", ops.torgb_small, x, wt, st, bs, rgb_in, None, y_pre)
    for bad_pre in (z(2, 3, 4, 5), z(1, 3, 4, 6), z(2, 3, 2, 3)):
        refuses("y_pre must be", ops.torgb_small, x, wt, st, bs, None, None, bad_pre)
    refuses("Cout=5", ops.torgb_small, x, z(5, 8), st, z(5), None, None, None)
    refuses("torgb_fwd failed", ops.torgb_small, z(2, 3, 6, 8), wt, st, bs, None, None, None)     # odd H
    refuses("torgb_fwd failed", ops.torgb_small, z(2, 4, 5, 8), wt, st, bs, None, None, None)     # odd W
    refuses("torgb_fwd failed", ops.torgb_small, z(2, 4, 6, 6), z(3, 6), z(2, 6), bs, None, None, None)      # Cin % 4 != 0
    # torgb_finish
    part = z(2, 2, 4, 6, 4)
    refuses("part must be", ops.torgb_finish, z(2, 2, 4, 6, 3), bs, None, None, y_pre)
    refuses("part must be", ops.torgb_finish, z(2, 4, 6, 4), bs, None, None, y_pre)
    refuses(r"bias \[Cout\]", ops.torgb_finish, part, z(3, 1), None, None, y_pre)
    refuses("rgb_in must be", ops.torgb_finish, part, bs, z(2, 3, 2, 2), None, y_pre)
    refuses("y_pre must be", ops.torgb_finish, part, bs, None, None, z(2, 3, 4, 5))
    refuses(r"Cout=4 \(max 3\)", ops.torgb_finish, part, z(4), None, None, None)
    refuses("torgb_finish_fwd failed", ops.torgb_finish, z(2, 2, 3, 6, 4), bs, None, None, None)  # odd H
    # styles
    w = z(2, 16)
    refuses("affine_w must be", ops.styles_demod, w, z(5, 12), z(5), None)
    refuses("affine_b must be", ops.styles_demod, w, z(5, 16), z(4), None)
    refuses("wsq must be", ops.styles_demod, w, z(5, 16), z(5), z(7, 4))
    refuses("wsq must be", ops.styles_demod_batch, [(w, z(5, 16), z(5), z(7, 6), 1.0, 1e-8)])
    refuses("affine_w must be", ops.styles_demod_batch, [(w, z(5, 16), z(5), None, 1.0, 1e-8), (w, z(5, 20), z(5), None, 1.0, 1e-8)])
    refuses("bad dims", ops.styles_demod, z(2, 6), z(5, 6), z(5), None)                           # w_dim % 4 != 0
    refuses("bad dims", ops.styles_demod_batch, [(z(2, 6), z(5, 6), z(5), None, 1.0, 1e-8)])
    refuses(r"1\.\.32 items", ops.styles_demod_batch, [(w, z(5, 16), z(5), None, 1.0, 1e-8)] * 33)
    assert len(cases) > 50
    torch.cuda.synchronize()
    assert (slots == 1).all() and (short == 1).all() and (y_pre == 1).all()

"""The conv GEMM kernels (csrc/modconv.hip, modconv_bf16.hip, smallconv.hip, upconv_fir.hip, upfir_lean.hip, torgb_skip.hip) against
the float64 reference of tests/conv_ref.py, route by route, one entry point at a time, in three tiers:

  exact      integer operands and dyadic scalars: every kind, loop, tile and split-K order equals the reference bit for bit (indexing,
             borders, ragged tiles, chunk pairs and tails, slabs, the epilogue at planted pre-activation values 0 and +-clamp / gain;
             at most 5 % of a clamped case's outputs sit on the clamp, and four cases in five run without one).
  multipart  bit for bit too, on operands that need their low parts: one sub-tier per part product a kind keeps
             (conv_ref.SUBTIERS), so a dropped, swapped or mis-indexed low-part product changes bits.
  realistic  randn inputs, style magnitudes 1e-2 .. 1e2 per sample: every element within
             (N + 16) u mag + e_kind mag (+ the absolute step of fp16 parts), conv_ref.kind_bound; the constants are derived
             there, never measured.  The worst error / bound per (route, kind) is printed and recorded in
             profiles/conv_kernels_f64.md.

Groups (conv_ref.cases): the fp32 staged kernel (four N tiles, five modes, split-K, broadcast x); the 16-bit staged 16-channel
loop (every kind; 3x3, 1x1 on the padded 96-channel tile with the pad poisoned, both adjoints; one pixel to ragged tiles; more
K slices than chunks); the 32-channel loops of f16x3 (one chunk, a pair, a pair and the odd tail; the per-call legacy switches;
fused toRGB with and without y; y_absmax; x_absmax); the small-image kernel (one and several K slices); the merged up-conv
(fringe tiles, a tile over three samples, more samples than staged, Cout 64 and 128, fp16 storage); upconv_fir (strip and
streaming kernels) and torgb_skip, each in all three tiers.  The switches the library reads once per process run in child processes (tests/conv_child.py).

Needs an MI355X:  python -m pytest tests/test_gpu_conv_kernels.py -m gpu"""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import conv_child as K
from tests import conv_ref as R
from tests.test_gpu_forward_kernels import hold_absmax

pytestmark = pytest.mark.gpu

WORST = {}                     # (route, kind) -> largest error / bound seen in the realistic tier
CASES = R.cases()
GROUPS = sorted({(c["group"], c["kind"]) for c in CASES})


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for key in sorted(WORST):
        print(f"\nworst error / bound [{key[0]} {key[1]}]: {WORST[key]:.4f}", end="")


def same_bits(got, ref, what, half=False):
    assert got.shape == ref.shape and got.dtype == (torch.float16 if half else torch.float32), what
    bad = K.differing(got, ref)
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the float64 reference"


def within(key, got, ref, bnd, what):
    r = R.ratio(got, ref, bnd)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, f"{key} {what}: error is {r:.3f} of the bound"


def slots_of(v, dev):
    s = torch.zeros(R.ABSMAX_SLOTS * R.ABSMAX_STRIDE, device=dev)
    s[0] = v
    return s


def rgb_of(part):
    return part.double().cpu().sum(0)[..., :3]


# ----------------------------------------------------------------------------- hfagp_modconv_fwd
@pytest.mark.parametrize("group,kind", GROUPS)
def test_modconv_exact(dev, group, kind):
    for c in (c for c in CASES if (c["group"], c["kind"]) == (group, kind)):
        t, q = R.inputs(c, "exact")
        ref, mag = R.modconv(batch=c["B"], **R.ref_kwargs(t), mode=c["mode"])
        R.exact_precondition(ref, mag, q, c["id"])
        R.planted(c, ref)
        xmax = slots_of(float(t["x"].abs().max()), dev) if c.get("x_absmax") else None
        out = K.run_modconv(c, t, dev, x_absmax=xmax)
        if c["rgb"]:
            y, part = out
            rgb, mrgb = R.fused_torgb(ref, mag, t["rgb_w"])
            R.exact_precondition(rgb, mrgb, q, c["id"])
            assert part.shape[0] == 2 * (c["Cout"] // 128) and (y is None) == (not c["store_y"]), c["id"]
            assert K.differing(rgb_of(part), rgb) == 0, f"{c['id']}: the fused toRGB sums differ from the float64 reference"
            out = y
        if out is not None:
            same_bits(out, ref, c["id"], half=c["y_f16"])
        if c.get("y_absmax"):
            hold_absmax(lambda slots: K.run_modconv(c, t, dev, y_absmax=slots), out, False, c["id"])


@pytest.mark.parametrize("group,kind", [g for g in GROUPS if R.SUBTIERS.get(g[1])])
def test_modconv_multipart(dev, group, kind):
    ran = 0
    for c in (c for c in CASES if (c["group"], c["kind"]) == (group, kind)):
        for sub in R.SUBTIERS[kind]:
            if not R.multipart_fits(c, sub):
                continue
            t, q = R.multipart_inputs(c, sub)
            what = f"{c['id']} {sub}"
            ref, mag = R.modconv(t["x"], t["weight"], c["mode"], t["styles"])
            R.exact_precondition(ref, mag, q, what)
            R.multipart_precondition(t, kind, sub, c["mode"], what)
            xmax = slots_of(2.0 ** 14, dev) if c.get("x_absmax") else None          # (2^14: the guard's scale of x stays 1)
            same_bits(K.run_modconv(c, t, dev, x_absmax=xmax), ref, what)
            ran += 1
    assert ran > 0


@pytest.mark.parametrize("group,kind", GROUPS)
def test_modconv_realistic(dev, group, kind):
    for c in (c for c in CASES if (c["group"], c["kind"]) == (group, kind)):
        t, _ = R.inputs(c, "realistic")
        if c["x_f16"]:
            t["x"] = t["x"].half().float()              # the reference reads the stored halves as they are
        ref, mag = R.modconv(batch=c["B"], **R.ref_kwargs(t), mode=c["mode"])
        xs = R.modulated(t["x"], t["styles"], c["mode"], c["B"])
        xam = float(t["x"].abs().max()) if c.get("x_absmax") else None
        bnd = R.kind_bound(t, kind, c["mode"], R._gemm(xs.abs(), t["weight"].double().abs(), c["mode"]), x_absmax=xam, x_f16=c["x_f16"])
        if c["mode"] in R.FUSED:
            bnd = R.epilogue_bound(bnd, t.get("dcoef"), t["gain"])
        bnd = R.full_bound(bnd, mag, R.terms(c["mode"], c["Cin"]))         # N = taps Cin + 3 (the epilogue), once
        if c["y_f16"]:                                 # the stored half: 2^-11 |ref|, or half a subnormal step
            bnd = bnd + torch.maximum(R.U16 * ref.abs(), torch.full_like(ref, 2.0 ** -25))
        key = (R.route(c, c["env"]), kind)
        out = K.run_modconv(c, t, dev, x_absmax=None if xam is None else slots_of(xam, dev))
        if c["rgb"]:
            y, part = out
            rgb, mrgb = R.fused_torgb(ref, mag, t["rgb_w"])
            brgb = R.fused_torgb(ref, bnd, t["rgb_w"])[1] + (c["Cout"] + 16) * R.U * mrgb
            within((key[0] + " toRGB", kind), rgb_of(part), rgb, brgb, c["id"])
            out = y
        if out is not None:
            assert out.dtype == (torch.float16 if c["y_f16"] else torch.float32), c["id"]
            within(key, out, ref, bnd, c["id"])


# ----------------------------------------------------------------------------- hfagp_upconv_fir_fwd
def run_fir(c, t, dev, slots=None):
    from hfa_gp_amd import ops
    on = lambda k: None if t.get(k) is None else t[k].to(dev)       # noqa: E731
    with K.switches(c["env"]):
        return ops.upconv_fir(t["x"].to(dev), K.image(t["weight"], c["kind"], dev), c["Cout"], on("styles"), on("dcoef"), on("noise"),
                              t["strength"], on("bias"), t["act"], t["alpha"], t["gain"], t["clamp"], y_absmax=slots)


@pytest.mark.parametrize("tier", R.TIERS)
@pytest.mark.parametrize("kernel", sorted(R.FIR_SHAPES))
def test_upconv_fir(dev, kernel, tier):
    """Strip kernel (Cin 48; Cin 32 with the streaming kernel switched off) and streaming kernel (Cin 32) at 9 x 20 -> 18 x 40, two
    strips of 32 y_t columns with a ragged second one; dcoef, noise, bias each present and absent, both activations, clamp on / off."""
    for c in R.fir_cases(kernel):
        t, q = R.fir_inputs(c, tier)
        ref, mag = R.upconv_fir(**t)
        if tier == "exact":
            R.exact_precondition(ref, mag, q, c["id"])
            R.fir_planted(c, t, ref)
            got = run_fir(c, t, dev)
            same_bits(got, ref, c["id"])
            if c["epi"] in (0, 7):
                hold_absmax(lambda slots: run_fir(c, t, dev, slots), got, False, c["id"])
        else:
            mt = R.modconv(t["x"], t["weight"], "up", t["styles"])[1]
            within((f"upconv_fir/{kernel}", c["kind"]), run_fir(c, t, dev), ref, R.fir_bound(t, c["kind"], mt), c["id"])


@pytest.mark.parametrize("kernel", sorted(R.FIR_SHAPES))
def test_upconv_fir_multipart(dev, kernel):
    """The low-part products of the strip and streaming kernels' own MFMA loops: every sub-tier of every kind they run, bit for bit."""
    for c, sub, t, q in R.fir_multipart(kernel):
        what = f"{c['id']} {sub}"
        ref, mag = R.upconv_fir(t["x"], t["weight"], t["styles"], act="linear", gain=1.0)
        R.exact_precondition(ref, mag, q, what)
        R.multipart_precondition(t, c["kind"], sub, "up", what)
        same_bits(run_fir(c, dict(t, strength=0.0, alpha=0.2), dev), ref, what)


# ----------------------------------------------------------------------------- hfagp_torgb_skip_fwd
def test_torgb_skip_multipart(dev):
    """The low-part products of torgb_skip_kernel's own MFMA loop: every sub-tier of f16x3, bf16x3 and bf16x6, bit for bit."""
    from hfa_gp_amd import ops
    for c, sub, t, q in R.skip_multipart():
        what = f"{c['id']} {sub}"
        ref, mag = R.torgb_skip(t["x"], t["weight"], t["styles"], t["bias"])
        R.exact_precondition(ref, mag, q, what)
        R.multipart_precondition(t, c["kind"], sub, "1x1", what)
        got = ops.torgb_skip(t["x"].to(dev), K.image(t["weight"], c["kind"], dev), c["Cout"], t["styles"].to(dev), t["bias"].to(dev), None)
        same_bits(got, ref, what)


@pytest.mark.parametrize("tier", R.TIERS)
@pytest.mark.parametrize("kind", R.SKIP_KINDS)
def test_torgb_skip(dev, kind, tier):
    """The streaming toRGB + skip kernel at its smallest supported shape, 1 x 128 x 128 x 16: Cout 32 and 96, with and without the
    half-resolution image, plain and plane-major stores."""
    from hfa_gp_amd import ops
    for c in (c for c in R.skip_cases() if c["kind"] == kind):
        t, q = R.skip_inputs(c, tier)
        ref, mag = R.torgb_skip(plane_major=c["plane_major"], **t)
        img = t["img"].to(dev) if c["img"] else None
        got = ops.torgb_skip(t["x"].to(dev), K.image(t["weight"], kind, dev), c["Cout"], t["styles"].to(dev), t["bias"].to(dev), img,
                             plane_major=c["plane_major"])
        if tier == "exact":
            R.exact_precondition(ref, mag, q, c["id"])
            same_bits(got, ref, c["id"])
            continue
        my = R.modconv(t["x"], t["weight"], "1x1", t["styles"])[1]
        # N = Cin + 3 (the conv and its bias) + 5 (four taps of the up-sampled image and the add), once
        bnd = R.full_bound(R.skip_upsample_add(None, R.kind_bound(t, kind, "1x1", my), c["plane_major"])[1], mag, R.SKIP_SHAPE[3] + 3 + 5)
        within(("torgb_skip", kind), got, ref, bnd, c["id"])


# ----------------------------------------------------------------------------- the read-once switches
def test_read_once_switches_in_child_processes():
    """HFAGP_DEV_UP_LEGACY_TILES, _UP_NO_FRINGE, _UP_WAVES=8 and _XCD_REMAP are read once per process: each runs the exact tier in a
    fresh process (tests/conv_child.py), one child at a time, each under its own time limit; a child that dies abnormally ends
    the test before another one starts.  Every child's result is the float64 reference bit for bit — the bits of the default
    plan, which test_modconv_exact holds to the same reference — under a plan that the library confirms differs."""
    root = Path(__file__).resolve().parents[1]
    for variant in K.VARIANTS:
        n = len(K.variant_cases(variant))
        # (a fresh process: ~20 s to load torch and the library and to create the context, well under 0.5 s per case)
        r = subprocess.run([sys.executable, "-m", "tests.conv_child", variant], cwd=root, capture_output=True, text=True,
                           timeout=60 + n)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("OK ", "MISMATCH "))]
        assert r.returncode in (0, 1), f"{variant}: the child ended abnormally ({r.returncode}); no further child is started\n{r.stderr[-2000:]}"
        assert r.returncode == 0 and len(lines) == n and all(ln.startswith("OK ") for ln in lines), \
            f"{variant}:\n" + "\n".join(ln for ln in lines if not ln.startswith("OK ")) + r.stderr[-2000:]

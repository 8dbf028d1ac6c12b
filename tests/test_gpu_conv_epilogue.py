"""The batched epilogue of the conv GEMM loops in csrc/modconv_bf16.hip against the form they replace (developer
switch HFAGP_DEV_CONV_EPILOGUE_LEGACY=1: the forward 3x3 conv at f16x3, on the 32-channel loop and — with
HFAGP_DEV_CONV9_LEGACY=1 — on the 16-channel one).  The operands of an output are fetched earlier and the stores are branch-free;
the arithmetic of an output and the order of every sum are unchanged, so the two forms must agree BIT FOR BIT: y, the fused toRGB
partial sums and the published max |y|.  Shapes: the smallest that reach every branch — B = 2 (dcoef and styles differ per sample),
one 32-channel chunk and the two-chunk pair, one and two N blocks (distinct rgb_part slabs), an exact 8 x 16 tile, one row and one
column over it (partial tiles beside full ones in both directions), and a single tile that is mostly outside the image.  ksplit is
given (1, or 2 for the slab stores and the reducer): left to the plan, images this small go to the small-image kernel."""
import math

import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


SETTINGS = {
    # noise (non-zero strength), dcoef, bias, clamp
    "noise_dcoef_bias_clamp": dict(noise=True, mod=True, clamp=1.5, absmax=False, rgb=False, store_y=True, ksplit=1),
    # nothing optional, no clamp, max |y| tracked
    "bare_absmax": dict(noise=False, mod=False, clamp=None, absmax=True, rgb=False, store_y=True, ksplit=1),
    # fused toRGB beside y (and max |y|), and alone
    "rgb_store_y": dict(noise=True, mod=True, clamp=None, absmax=True, rgb=True, store_y=True, ksplit=1),
    "rgb_only": dict(noise=True, mod=True, clamp=1.5, absmax=False, rgb=True, store_y=False, ksplit=1),
    # split K: unfused slab stores in the kernel (one slice is empty at Cin = 32 on the 32-channel loop), epilogue in the reducer
    "ksplit2": dict(noise=True, mod=True, clamp=1.5, absmax=True, rgb=False, store_y=True, ksplit=2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("loop16", [False, True], ids=["loop32", "loop16"])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("H,W", [(8, 16), (9, 17), (3, 5)])
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [32, 64])
def test_conv_epilogue_bits(dev, monkeypatch, cin, cout, H, W, setting, loop16):
    from hfa_gp_amd import ops
    cfg = SETTINGS[setting]
    B = 2
    g = torch.Generator(device=dev).manual_seed(1000 * cin + 10 * cout + H)
    x = torch.randn(B, H, W, cin, device=dev, generator=g)
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) / math.sqrt(9 * cin)
    s = torch.randn(B, cin, device=dev, generator=g) + 1.0
    dcoef = torch.rand(B, cout, device=dev, generator=g) + 0.5
    bias = torch.randn(cout, device=dev, generator=g)
    noise = torch.randn(H, W, device=dev, generator=g)
    rgb_w = torch.randn(B, 3, cout, device=dev, generator=g) / math.sqrt(cout)
    wt = ops.weight_prep_prec(w, "f16x3")

    def run():
        slots = ops.absmax_slots(1, dev)
        out = ops.modconv(x, wt, cout, ops.CONV3X3, styles=s, dcoef=dcoef if cfg["mod"] else None,
                          noise=noise if cfg["noise"] else None, noise_strength=0.3 if cfg["noise"] else 0.0,
                          bias=bias if cfg["mod"] else None, act="lrelu", gain=math.sqrt(2), clamp=cfg["clamp"],
                          ksplit=cfg["ksplit"], y_absmax=slots[0] if cfg["absmax"] else None,
                          rgb_w=rgb_w if cfg["rgb"] else None, store_y=cfg["store_y"])
        y, part = out if cfg["rgb"] else (out, None)
        torch.cuda.synchronize()
        return y, part, slots.max().item()

    if loop16:
        monkeypatch.setenv("HFAGP_DEV_CONV9_LEGACY", "1")
    else:
        monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY", raising=False)
    monkeypatch.delenv("HFAGP_DEV_CONV_EPILOGUE_LEGACY", raising=False)
    y_new, p_new, m_new = run()
    monkeypatch.setenv("HFAGP_DEV_CONV_EPILOGUE_LEGACY", "1")
    y_old, p_old, m_old = run()

    if cfg["store_y"]:
        assert y_new.shape == (B, H, W, cout) and torch.isfinite(y_new).all()
        assert y_new.abs().max().item() > 0.1             # (a kernel that stored nothing would agree with itself as well)
        assert torch.equal(y_new, y_old)
    else:
        assert y_new is None and y_old is None
    if cfg["rgb"]:
        assert p_new.shape == p_old.shape and p_new.shape[0] == cout // 64
        assert torch.isfinite(p_new).all() and p_new[..., :3].abs().max().item() > 0.01
        assert torch.equal(p_new, p_old)
    if cfg["absmax"]:
        assert m_new == m_old
        assert m_new == y_new.abs().max().item()         # max is exact: the slot holds the largest stored |y|, not an estimate

"""`ops.fused_torgb_supported` / `ops.f16_storage_supported` answer with the library's own launch plan
(`hfagp_modconv_workspace_bytes(args) == 0`: no split-K, epilogue in the conv kernel — include/hfagp.h) instead of a copy of its
arithmetic.  Host-only planning: no compute call is made, so no GPU is needed (the library is loaded as in test_abi.py).

The sweep pins them to the formulas they replace, written out literally below, wherever those were right:

  * `f16_storage_supported` == `cin < 64 or blocks >= 129` on every point.  The predicate takes no mode: it vouches for the 3x3 conv
    AND the up-sampling conv of a super-resolution block, so it is true where the library splits NEITHER call.  For the 3x3 call
    that is the retired expression exactly; the up-sampling call's merged four-phase grid has more blocks than the expression
    counts, so on 33 of the 240 points (e.g. B = 1, 128^2, 128 -> 128) the library would not split it although the 3x3 call of
    the same shape is split — there the predicate stays False, as the expression did (`up_only` below counts them).
  * `fused_torgb_supported` == `blocks >= 129` on every point with cin >= 64 (every conv1 of every shipped config).
  * `fused_torgb_supported` with cin < 64: the retired formula lacked the `cin < 64` clause of its twin (a K range of fewer than four
    16-channel chunks is never split); it now says what the library says — the one intended difference, asserted point by point.
"""
import ctypes as C
import itertools
import os

import pytest
import torch

BATCHES = (1, 2, 5, 8, 32)
SIDES = (8, 16, 24, 32, 40, 64, 128, 256)
CHANNELS = ((32, 128), (64, 128), (128, 128), (256, 128), (256, 256), (512, 512))
POINTS = list(itertools.product(BATCHES, SIDES, CHANNELS))


@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    return _lib


def blocks_of(b, h, w, cout):
    return b * ((h + 7) // 8) * ((w + 15) // 16) * (cout // 128)


def unsplit(lib, mode, b, h, w, cin, cout, precision, x_f16=0, y_f16=0, rgb=False):
    """hfagp_modconv_workspace_bytes() == 0 for the args of the real call, filled in by hand (not through ops._modconv_args)."""
    a = lib.ModconvArgs()
    a.x = a.wt = a.y = 1                        # non-null, never dereferenced by planning
    a.rgb_w = 1 if rgb else None
    a.B, a.H, a.W, a.Cin, a.Cout = b, h, w, cin, cout
    a.mode, a.precision, a.x_f16, a.y_f16 = mode, precision, x_f16, y_f16
    a.x_batch_stride = h * w * cin
    a.alpha, a.gain, a.clamp = 0.2, 1.0, 256.0
    return lib.lib().hfagp_modconv_workspace_bytes(C.byref(a)) == 0


def test_workspace_query_needs_no_device(lib):
    from hfa_gp_amd import ops
    assert unsplit(lib, ops.CONV3X3, 32, 64, 64, 128, 128, ops.PREC_F16X3)
    assert not unsplit(lib, ops.CONV3X3, 1, 8, 8, 128, 128, ops.PREC_F16X3, rgb=True)
    assert unsplit(lib, ops.CONVT3X3_UP2, 32, 64, 64, 128, 128, ops.PREC_F16, y_f16=1)
    assert not unsplit(lib, ops.CONVT3X3_UP2, 1, 8, 8, 128, 128, ops.PREC_F16, y_f16=1)


def test_f16_storage_supported_is_the_librarys_answer(lib):
    from hfa_gp_amd import ops
    up_only = 0
    for b, s, (cin, cout) in POINTS:
        got = ops.f16_storage_supported(s, s, cin, cout, b)
        retired = cin < 64 or b * ((s + 7) // 8) * ((s + 15) // 16) * (cout // 128) >= 129
        assert got == retired, (b, s, cin, cout)
        conv = unsplit(lib, ops.CONV3X3, b, s, s, cin, cout, ops.PREC_F16, 1, 1)
        # the up-sampling conv of a block reads fp32 (first super-resolution layer) or fp16 activations
        up = [unsplit(lib, ops.CONVT3X3_UP2, b, s, s, cin, cout, ops.PREC_F16, x_f16, 1) for x_f16 in (1, 0)]
        assert up[0] == up[1], (b, s, cin, cout)
        assert got == conv, (b, s, cin, cout)                   # CONV3X3: predicate <=> the real call is not split
        assert got == (conv and up[0]), (b, s, cin, cout)       # both calls it vouches for: true <=> neither is split
        up_only += up[0] and not conv
    assert up_only == 33
    assert not ops.f16_storage_supported(64, 64, 24, 128, 32) and not ops.f16_storage_supported(64, 64, 64, 96, 32)


@pytest.mark.parametrize("precision", ["f16x3", "f16", "bf16x3", "bf16x6"])
def test_fused_torgb_supported_is_the_librarys_answer(lib, precision):
    from hfa_gp_amd import ops
    images = {}
    differs = 0
    for b, s, (cin, cout) in POINTS:
        # (host tensors stand for the device ones: the predicate reads shapes and dtypes and passes addresses on; expand(): no memory)
        x = torch.empty(1, s, s, cin).expand(b, s, s, cin)
        wt = images.setdefault((cin, cout), torch.empty(ops.NPARTS[precision], 9, cin // 8, cout, 8, dtype=ops._IMAGE_DTYPE[precision]))
        got = ops.fused_torgb_supported(x, wt, cout, b)
        assert got == unsplit(lib, ops.CONV3X3, b, s, s, cin, cout, ops.PRECISIONS[precision], rgb=True), (b, s, cin, cout)
        retired = b * ((s + 7) // 8) * ((s + 15) // 16) * (cout // 128) >= 129
        if cin >= 64:
            assert got == retired, (b, s, cin, cout)
        else:
            # the intended difference: fewer than four 16-channel K chunks are never split, whatever the grid
            assert got is True, (b, s, cin, cout)
            differs += got != retired
    assert differs == 25                # the cin = 32 points below 129 blocks, which the retired formula refused
    assert not ops.fused_torgb_supported(torch.empty(32, 64, 64, 128), torch.empty(9, 32, 128, 4), 128, 32)      # fp32 image
    wt96 = torch.empty(ops.NPARTS[precision], 9, 16, 96, 8, dtype=ops._IMAGE_DTYPE[precision])
    assert not ops.fused_torgb_supported(torch.empty(32, 64, 64, 128), wt96, 96, 32)


def test_a_broadcast_input_is_planned_as_such(lib):
    """x [1, H, W, Cin] with batch > 1 (the learned constant): the same answer as the full batch here, under its own memo key."""
    from hfa_gp_amd import ops
    wt = torch.empty(2, 9, 16, 128, 8, dtype=torch.float16)
    for b, s in ((1, 8), (32, 8), (32, 64)):
        one, full = torch.empty(1, s, s, 128), torch.empty(1, s, s, 128).expand(b, s, s, 128)
        assert ops.fused_torgb_supported(one, wt, 128, b) == ops.fused_torgb_supported(full, wt, 128, b) == (blocks_of(b, s, s, 128) >= 129)
    assert any(k[-1] for k in ops._PLAN_UNSPLIT) and not all(k[-1] for k in ops._PLAN_UNSPLIT)

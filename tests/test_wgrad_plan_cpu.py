"""The weight gradient's host plan (csrc/wgrad_plan.h): `hfagp_wgrad_ksplit` and `hfagp_wgrad_workspace_bytes` against the formula
written out literally below, and `tests/backward_ref.wgrad_split16` against its `split16` term.  Host-only planning: no compute
call is made, so no GPU is needed (the library is loaded as in test_plan_predicates.py)."""
import ctypes as C
import itertools
import os

import pytest

from tests import backward_ref as R

BATCHES = (1, 2, 32)
HEIGHTS = (4, 9, 64, 256)                       # W = H + 1
CHANNELS = ((4, 32), (8, 32), (24, 96), (32, 128), (64, 64), (96, 96), (256, 128), (512, 512))
MODES = ("3x3", "up", "1x1")
PRECISIONS = ("fp32", "bf16x3")
POINTS = list(itertools.product(BATCHES, HEIGHTS, CHANNELS, MODES, PRECISIONS))


@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    return _lib


def ceil_div(a, b):
    return -(-a // b)


def test_ksplit_and_workspace_follow_the_written_formula(lib):
    from hfa_gp_amd import ops
    mode_of = {"3x3": ops.CONV3X3, "up": ops.CONVT3X3_UP2, "1x1": ops.CONV1X1}
    prec_of = {"fp32": ops.PREC_F32, "bf16x3": ops.PREC_BF16X3}
    assert len(POINTS) == 576
    taken = 0
    for b, h, (cin, cout), mode, prec in POINTS:
        w = h + 1
        split16 = prec == "bf16x3" and mode in ("3x3", "up") and cout % 64 == 0 and (cin % 64 == 0 or (mode == "up" and cin == 32))
        rows = 4 if split16 else 2
        units = b * ceil_div(h, rows) * ceil_div(w, 16)
        tiles = ceil_div(cin, 64) * ceil_div(cout, 64)
        k = min(max(max(1, (256 if split16 else 512) // tiles), 1), min(units, 256))
        nbytes = k * (1 if mode == "1x1" else 9) * cin * cout * 4

        a = lib.WgradArgs()
        a.B, a.H, a.W, a.Cin, a.Cout = b, h, w, cin, cout
        a.mode, a.precision = mode_of[mode], prec_of[prec]
        point = (b, h, w, cin, cout, mode, prec)
        got = lib.lib().hfagp_wgrad_ksplit(C.byref(a))
        assert got == k, point
        a.ksplit = got
        assert lib.lib().hfagp_wgrad_workspace_bytes(C.byref(a)) == nbytes, point
        assert R.wgrad_split16((b, h, w, cin, cout), prec, mode) == split16, point
        taken += split16
    assert 0 < taken < len(POINTS)


def test_plan_queries_refuse_nothing_and_need_no_device(lib):
    a = lib.WgradArgs()                          # all zero: the policy answers 1 slab, the workspace query 0 bytes
    assert lib.lib().hfagp_wgrad_ksplit(C.byref(a)) == 1
    assert lib.lib().hfagp_wgrad_workspace_bytes(C.byref(a)) == 0

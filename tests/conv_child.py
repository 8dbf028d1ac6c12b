"""The conv kernels behind the developer switches that the library reads ONCE per process (`static` in make_plan, csrc/modconv_plan.h):
    python -m tests.conv_child VARIANT          VARIANT in legacy_tiles, no_fringe, waves8, xcd
runs the exact-tier up-conv and 3x3 cases of tests/conv_ref.py in this (fresh) process with the variant's switch set, prints one
line per case and exits non-zero on any element that differs from the float64 reference.  For every case it also asks the library
for its workspace under the switch and compares with the predictor (`conv_ref.plan` with the same switch): the plan the switch
asks for is the one in force.  tests/test_gpu_conv_kernels.py starts the four variants one after another.

Also the device-side runners the GPU tests share (`run_modconv`)."""
import contextlib
import ctypes as C
import os
import sys

import torch

from tests import conv_ref as R

VARIANTS = {"legacy_tiles": {"HFAGP_DEV_UP_LEGACY_TILES": "1"}, "no_fringe": {"HFAGP_DEV_UP_NO_FRINGE": "1"},
            "waves8": {"HFAGP_DEV_UP_WAVES": "8"}, "xcd": {"HFAGP_DEV_XCD_REMAP": "1"}}


def variant_cases(variant):
    """The up-conv and 3x3 cases without a per-call switch; the 8-wave block: the up-conv at Cout 128, every kind but bf16x6."""
    cs = [c for c in R.cases() if c["mode"] in ("up", "3x3") and c["group"] in ("up", "loop32", "staged16") and not c["env"]]
    if variant == "waves8":
        cs = [c for c in cs if c["mode"] == "up" and c["Cout"] % 128 == 0 and c["kind"] != "bf16x6"]
    elif variant != "xcd":
        cs = [c for c in cs if c["mode"] == "up"]
    return cs


@contextlib.contextmanager
def switches(env):
    """The per-call developer switches of one case, set for the duration of its launches."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def image(weight, kind, dev):
    """The weight image of one kind; behind a 16-bit image whose Cout is no multiple of 128 the 512-byte pad is poisoned (the
    128-wide tile reads it and must discard what it computes from it)."""
    from hfa_gp_amd import ops
    w = weight.to(dev)
    if kind == "fp32":
        return ops.weight_prep(w)[0]
    wb = ops.weight_prep_prec(w, "f16x3" if kind == "f16x2" else kind)
    if weight.shape[0] % 128:
        whole = torch.empty(0, dtype=wb.dtype, device=dev).set_(wb.untyped_storage())
        assert whole.numel() == wb.numel() + 256, "the 512-byte pad behind the image is gone: nothing to poison"
        whole[wb.numel():] = float("nan")
    return wb


def run_modconv(c, t, dev, x_absmax=None, y_absmax=None):
    """ops.modconv of one case on the tensors of conv_ref.inputs: y, or (y | None, rgb_part) with the fused toRGB."""
    from hfa_gp_amd import ops
    x = t["x"].to(dev)
    on = lambda k: None if t.get(k) is None else t[k].to(dev)       # noqa: E731
    with switches(c["env"]):
        return ops.modconv(x.half() if c["x_f16"] else x, image(t["weight"], c["kind"], dev), c["Cout"], R.MODE_ID[c["mode"]],
                           styles=on("styles"), dcoef=on("dcoef"), noise=on("noise"), noise_strength=t.get("strength", 0.0),
                           bias=on("bias"), act=t.get("act", "linear"), alpha=t.get("alpha", 0.2), gain=t.get("gain", 1.0),
                           clamp=t.get("clamp"), batch=c["B"], ksplit=c["ksplit"], x_absmax=x_absmax, y_absmax=y_absmax,
                           rgb_w=on("rgb_w"), y_f16=c["y_f16"], store_y=c.get("store_y", True), x_parts=int(c["kind"] == "f16x2"))


def differing(got, ref):
    return int((got.double().cpu() != ref).sum().item())


def workspace_bytes(c, ksplit):
    from hfa_gp_amd import _lib, ops
    a = _lib.ModconvArgs()
    a.x = a.wt = a.y = 1                        # non-null, never dereferenced by planning
    a.rgb_w = 1 if c["rgb"] else None           # (the kernel choice reads it)
    a.B, a.H, a.W, a.Cin, a.Cout = (c[k] for k in ("B", "H", "W", "Cin", "Cout"))
    a.mode, a.precision, a.ksplit = R.MODE_ID[c["mode"]], ops.PRECISIONS[c["kind"]], ksplit
    a.x_f16, a.y_f16 = int(c["x_f16"]), int(c["y_f16"])
    a.x_batch_stride = c["H"] * c["W"] * c["Cin"]
    a.alpha, a.gain, a.clamp = 0.2, 1.0, 256.0
    return _lib.lib().hfagp_modconv_workspace_bytes(C.byref(a))


def main(variant):
    env = VARIANTS[variant]
    os.environ.update(env)                       # before the library's first plan
    from hfa_gp_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    bad = 0
    for c in variant_cases(variant):
        t, q = R.inputs(c, "exact")
        ref, mag = R.modconv(batch=c["B"], **R.ref_kwargs(t), mode=c["mode"])
        R.exact_precondition(ref, mag, q, c["id"])
        got = run_modconv(c, t, dev)
        if c["rgb"]:                               # (y | None, rgb_part): the fused toRGB sums count too
            n = differing(got[1].double().cpu().sum(0)[..., :3], R.fused_torgb(ref, mag, t["rgb_w"])[0])
            n += differing(got[0], ref) if got[0] is not None else 0
        else:
            n = differing(got, ref)
        plans = all(workspace_bytes(c, ks) == R.plan(dict(c, ksplit=ks), env)["ws_bytes"] for ks in (0, c["ksplit"]))
        bad += (n != 0) + (not plans)
        print(f"{'OK' if n == 0 and plans else 'MISMATCH'} {variant} {c['id']} {R.route(c, env)} differing={n} plan={'ok' if plans else 'DIFFERS'}",
              flush=True)
    torch.cuda.synchronize()
    print(f"{variant}: {bad} bad cases")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))

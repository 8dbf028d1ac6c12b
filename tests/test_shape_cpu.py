"""Shape export without a GPU: the MRC2014 writer, EG3D's volume post-processing, the CLI's arguments, and the point-query
kernel's build-time resources (no scratch, no spills in any instance)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_save_mrc_round_trip(tmp_path):
    from hfa_gp_amd.render import save_mrc
    rng = np.random.default_rng(0)
    vol = rng.standard_normal((4, 5, 6)).astype(np.float32)         # [NZ][NY][NX]
    path = tmp_path / "v.mrc"
    save_mrc(path, vol, voxel_size=0.25)
    raw = path.read_bytes()
    assert len(raw) == 1024 + vol.size * 4
    w = np.frombuffer(raw[:1024], dtype="<i4")
    f = np.frombuffer(raw[:1024], dtype="<f4")
    assert tuple(w[0:3]) == (6, 5, 4) and w[3] == 2                  # NX NY NZ, MODE 2
    assert tuple(w[7:10]) == (6, 5, 4)                               # MX MY MZ
    assert np.allclose(f[10:13], (1.5, 1.25, 1.0)) and np.all(f[13:16] == 90.0)
    assert tuple(w[16:19]) == (1, 2, 3)                              # MAPC MAPR MAPS
    assert f[19] == vol.min() and f[20] == vol.max() and np.isclose(f[21], vol.mean(dtype=np.float64), atol=1e-6)
    assert np.isclose(f[54], vol.std(dtype=np.float64), rtol=1e-5)  # RMS
    assert w[22] == 1 and w[23] == 0 and w[27] == 20140             # ISPG, NSYMBT, NVERSION
    assert raw[208:212] == b"MAP " and raw[212:216] == bytes((0x44, 0x44, 0, 0))
    back = np.frombuffer(raw[1024:], dtype="<f4").reshape(w[2], w[1], w[0])
    assert np.array_equal(back, vol)


def test_shape_volume_eg3d_flip_and_trim():
    from hfa_gp_amd.render import shape_volume_eg3d
    n = 64
    g = torch.arange(n ** 3, dtype=torch.float32).view(n, n, n)
    v = shape_volume_eg3d(g)
    pad = int(30 * n / 256)                                          # 7
    assert v.dtype == np.float32 and v.shape == (n, n, n) and pad == 7
    inner = v[pad:n - pad, pad:n - pad, pad:n - pad]
    want = np.flip(g.numpy(), 0)[pad:n - pad, pad:n - pad, pad:n - pad]
    assert np.array_equal(inner, want)
    for axis in range(3):
        for sl in (slice(0, pad), slice(n - pad, n)):
            idx = [slice(None)] * 3
            idx[axis] = sl
            assert np.all(v[tuple(idx)] == -1000)
    assert v[pad, pad, pad] == g[n - 1 - pad, pad, pad]
    with pytest.raises(ValueError):
        shape_volume_eg3d(torch.zeros(4, 4, 5))


def test_extract_shapes_cli_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import extract_shapes as X
    finally:
        sys.path.pop(0)
    a = X.build_parser().parse_args(["--seeds", "0-2,7", "--outdir", "o", "--resolution", "128"])
    assert a.seeds == [0, 1, 2, 7] and a.resolution == 128 and a.preset == "ffhq512_128" and a.ws is None
    a = X.build_parser().parse_args(["--ws", "w.npy", "--outdir", "o", "--preset", "tiny14"])
    assert a.ws == "w.npy" and a.seeds is None and a.resolution == 512
    with pytest.raises(SystemExit):
        X.build_parser().parse_args(["--outdir", "o"])                # a latent source is required
    with pytest.raises(SystemExit):
        X.build_parser().parse_args(["--seeds", "1", "--ws", "w.npy", "--outdir", "o"])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_shapes.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--resolution" in out.stdout and "--seeds" in out.stdout


def test_planes_query_binding_matches_header():
    """The ctypes image of HfagpPlanesQueryArgs has the header's field order (a reordering would not fail to load)."""
    from hfa_gp_amd import _lib
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpPlanesQueryArgs;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.PlanesQueryArgs._fields_]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_planes_query_kernel_has_no_scratch(tmp_path):
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\bplanes_query\b", build, re.M), "planes_query.hip is not in build.sh's unit list"
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-fno-vectorize",
                          "-c", os.path.join(ROOT, "hfa-gp_amd", "csrc", "planes_query.hip"), "-o", str(tmp_path / "x.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, set()
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name and "planes_query_kernel" in name:
            seen.add(name)
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert len(seen) == 8, seen          # {split fp16, fp32 decoder} x {rgb, sigma only} x {explicit, grid}


# units appended to build.sh's list since ABI 13 that this file holds to the packed-fp32 rule, with a kernel each must contain
# (test_kernel_resources.py pins the list before them)
APPENDED_UNITS = [("planes_query", "planes_query_kernel"), ("weight_prep", "weight_prep_batch_kernel")]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
@pytest.mark.parametrize("unit,kernel", APPENDED_UNITS, ids=[u for u, _ in APPENDED_UNITS])
def test_appended_unit_has_no_packed_fp32_arithmetic(tmp_path, unit, kernel):
    """test_kernel_resources.py's rule for every unit (build.sh's note on the lost low half of packed fp32 ops): compiled with build.sh's
    flags, the unit contains no v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\b%s\b" % unit, build, re.M), f"{unit}.hip is not in build.sh's unit list"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    asm = tmp_path / "unit.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", unit + ".hip"),
                          "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    assert kernel in text
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)

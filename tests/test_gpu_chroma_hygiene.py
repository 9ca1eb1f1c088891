"""Kernel hygiene of the chroma-layout entry points (chroma.hip), with the
helpers and the five steps of tests/hygiene.py (tests/test_gpu_kernel_hygiene.py
explains them).

These launchers take the NHWC frame as scalars (base, H, W, cstride, coff), so
the walk of test_gpu_kernel_hygiene.py, which looks for tensor-struct
parameters, does not see them; the table below covers them and a CPU test walks
chroma.hip and hip.CHROMA_SYMBOLS for an entry point it misses.

Per entry: every layout (4:4:4, 4:2:2, 4:2:0) at 8 bits and at 10; the frame
view sits inside a larger buffer (32 guard rows above and below, 8 lead and 8
tail channels), raw buffers have 64 guard elements on both sides; the
surroundings hold zero, all-ones NaN bits and 1e30 (integer buffers: the
type's minimum and maximum); outputs are pre-filled with NaN inside and a
canary around.  The results equal the restatement (tests/chroma_ref.py), are
bit-identical across the three fills, across two runs and after
dcvc_debug_poison_lds / dcvc_debug_poison_vgpr, no byte outside a view is
written and no output element is left unwritten.
"""
import os
import re

import numpy as np
import pytest
import torch

from dcvc_amd import hip as K
from tests import chroma_ref as C
from tests import hygiene as HY
from tests.hygiene import seeded

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = (38, 54, 48, 64)      # h, w, H, W: odd half-planes, padding on both axes, more than one block
LAYOUTS = ((1, 1), (2, 1), (2, 2))
DEPTHS = (8, 10)
TOL_SSE = 1e-12               # tests/test_frame16.py (rtol)
TABLE = {}


def entry(name, symbol, fn):
    assert name not in TABLE
    TABLE[name] = (fn, (symbol,))


def smp(E, key, d, *shape):
    """Samples in [0, max_val] as the device tensors hold them: uint8, or the
    bits of uint16 as int16."""
    def make():
        a = torch.randint(0, 1 << d, shape, generator=seeded(f"{key}{d}")).numpy()
        return torch.from_numpy(a.astype(np.uint8) if d == 8 else a.astype(np.uint16).view(np.int16))
    return E.const(f"{key}{d}{shape}", make)


def host(t, d):
    return t.numpy() if d == 8 else t.numpy().view(np.uint16)


def bits(a, d):
    """A sample array as the flat tensor an output buffer holds."""
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a if d == 8 else a.view(np.int16))


def hwc(a):
    """(H, W, C) numpy -> (1, C, H, W) fp64 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).unsqueeze(0).double()


def planes(E, d, sub):
    h, w, _, _ = FRAME
    return smp(E, "y", d, h, w), smp(E, "uv", d, 2, h // sub[1], w // sub[0])


def ingest_case(E, d, sub):
    h, w, H, W = FRAME
    yp, uv = planes(E, d, sub)
    out = E.y("y", 3, H, W)
    E.launch(K.yuvp_to_nhwc, E.raw(yp), E.raw(uv), h, w, d, sub, out)
    E.ref("y", lambda: hwc(C.ingest_yuv(host(yp, d), host(uv, d), d, sub, H, W)), None)


def ingest_rgb_case(E, d, sub):
    h, w, H, W = FRAME
    yp, uv = planes(E, d, sub)
    out = E.y("y", 3, H, W)
    pl = E.yraw("planes", 3 * h * w, torch.float32)
    E.launch(K.yuvp_to_rgb_nhwc, E.raw(yp), E.raw(uv), h, w, d, sub, out, pl)
    ref = lambda: C.ingest_rgb(host(yp, d), host(uv, d), d, sub, H, W)  # noqa: E731
    E.ref("y", lambda: hwc(ref()[0]), None)
    E.ref("planes", lambda: torch.from_numpy(ref()[1]).reshape(-1), None)


def sse_case(E, d, sub):
    """The three sums to rtol 1e-12, x_hat clamped in place over the whole view."""
    h, w, H, W = FRAME
    yp, uv = planes(E, d, sub)
    xh = E.const("xh", lambda: torch.rand(1, 3, H, W, generator=seeded("xh")) * 1.4 - 0.2)
    xa = E.inout("x_hat", xh)
    ws = E.scratch(int(K.lib().dcvc_frame_sse_workspace()) // 8, torch.float64) if not E.dry else None
    out = E.yraw("sse", 3, torch.float64)
    crop = np.ascontiguousarray(xh.clamp(0, 1)[0, :, :h, :w].numpy())
    E.launch(K.yuvp_sse, xa, E.raw(yp), E.raw(uv), h, w, d, sub, ws, out)
    E.ref("sse", lambda: torch.from_numpy(C.sse_yuv(crop, host(yp, d), host(uv, d), d, sub)), TOL_SSE, "rtol")
    E.ref("x_hat", lambda: xh.clamp(0, 1).double(), None)


def recon_case(E, d, sub, from_rgb):
    h, w, H, W = FRAME
    xh = E.const("xh", lambda: torch.rand(1, 3, H, W, generator=seeded("xh")) * 1.2 - 0.1)
    out = E.yraw("smp", sum(C.frame_sizes(h, w, sub)), torch.uint8 if d == 8 else torch.int16)
    E.launch(K.recon_to_yuvp, E.x(xh), h, w, d, sub, from_rgb, out)
    crop = np.ascontiguousarray(xh[0, :, :h, :w].numpy())
    E.ref("smp", lambda: bits(C.file_frame(crop, d, sub, from_rgb), d), None)


for _sub in LAYOUTS:
    for _d in DEPTHS:
        _tag = f"{_sub[0]}x{_sub[1]}, {_d} bit"
        entry(f"yuvp_to_nhwc {_tag}", "dcvc_yuvp_to_nhwc", lambda E, d=_d, s=_sub: ingest_case(E, d, s))
        entry(f"yuvp_to_rgb_nhwc {_tag}", "dcvc_yuvp_to_rgb_nhwc", lambda E, d=_d, s=_sub: ingest_rgb_case(E, d, s))
        entry(f"yuvp_sse {_tag}", "dcvc_yuvp_sse", lambda E, d=_d, s=_sub: sse_case(E, d, s))
        for _rgb in (False, True):
            entry(f"recon_to_yuvp {'from rgb' if _rgb else 'from yuv'} {_tag}", "dcvc_recon_to_yuvp",
                  lambda E, d=_d, s=_sub, r=_rgb: recon_case(E, d, s, r))


# ---------------------------------------------------------------- the tests
def entry_points():
    """The launchers this table answers for: the extern "C" functions of
    chroma.hip and hip.CHROMA_SYMBOLS."""
    text = open(os.path.join(ROOT, "dcvc_amd", "csrc", "hip", "chroma.hip")).read()
    return set(re.findall(r'extern "C" \w+ (dcvc_\w+)\(', text)) | set(K.CHROMA_SYMBOLS)


def test_every_chroma_launcher_has_a_hygiene_case():
    covered = {}
    for name, (_, syms) in TABLE.items():
        for s in syms:
            covered.setdefault(s, []).append(name)
    known = {n for n, _, _ in K.HIP_SYMBOLS}
    names = entry_points()
    assert len(names) == 4 and names <= known, sorted(names - known)
    missing = sorted(names - set(covered))
    assert not missing, f"chroma launchers without a hygiene case: {missing}"
    assert set(covered) <= known
    for s in names:                                   # every layout at 8 bits and above
        for sx, sy in LAYOUTS:
            for d in DEPTHS:
                assert any(f"{sx}x{sy}, {d} bit" in n for n in covered[s]), (s, sx, sy, d)
    # none of them is visible to the tensor-struct walk of test_gpu_kernel_hygiene.py
    for n, _, args in K.HIP_SYMBOLS:
        if n in names:
            assert K.CTensor not in args, n
    assert (HY.ROWS, HY.LEAD, HY.TAIL, HY.GUARD) == (32, 8, 8, 64)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_entry_builds_on_the_cpu(name):
    """Every entry builds its call and its references without a device (the
    launches skipped): each reference has the shape of the output it is for."""
    fn, _ = TABLE[name]
    env = HY.Env("zero", {}, device=torch.device("cpu"), dry=True)
    fn(env)
    assert env.refs and set(env.refs) <= set(env.outs)
    for out, (ref, _, _) in env.refs.items():
        r = ref()
        assert tuple(r.shape) == tuple(env.values(out).shape), (out, tuple(r.shape))


@gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_kernel_hygiene(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fn, syms = TABLE[name]
    try:
        routes = HY.run_entry(fn, name)
    finally:
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:     # a GPU error poisons the process: launch nothing more
            pytest.exit(f"GPU error, stopping: {e}", returncode=3)
    assert set(routes) == set(syms), (routes, syms)

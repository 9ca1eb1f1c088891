"""Which kernel dcvc_conv2d launches for which call, pinned.

The split-family launchers (tconv, nconv, wconv, xconv, dconv, sconv / sgemm)
and the bf16 / fp32 dispatcher decline a call by returning "unsupported", and
the next kernel in line computes the same values, only slower: a launcher that
starts to refuse a view or a shape it used to take fails no numerical test.
So every case below records dcvc_last_kernel() after the call (the whole
string, "@threads" suffix included, i.e. instantiation and grid) or the error
the call raised, and compares it with tests/golden/conv_routing.json.

DCVC_RECORD_ROUTING=1 rewrites the golden file from the library under test
instead of comparing (off by default).
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routing.json")
RECORD = os.environ.get("DCVC_RECORD_ROUTING", "0") == "1"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def K():
    from dcvc_amd import hip
    return hip


def C(name, cin, cout, k=3, s=1, H=32, W=48, **kw):
    """One case.  Keywords: compute ("f16x3" | "bf16" | "f32"), dt (dtype of
    the views: "f32" | "bf16"), ydt (of y alone), nres, shuf, gate, act slope
    `slope` (None: no activation), input leaky ReLU slope `in_slope`, xoff
    (input window offset in a wider buffer), ypad (extra channels of the
    output buffer), roff (residual window offset), res2_only, opts."""
    return dict(name=name, cin=cin, cout=cout, k=k, s=s, H=H, W=W, **kw)


# ---- all-aligned baselines, one per family and instantiation path
BASE = [
    C("tconv_3x3_2to32", 2, 32),
    C("tconv_3x3_2to64", 2, 64),
    C("tconv_1x1s2_2to128_lrelu", 2, 128, 1, 2, in_slope=0.1, act=0.1),
    C("nconv_7x7_16to2", 16, 2, 7),
    C("nconv_7x7_32to2", 32, 2, 7),
]
BASE += [C(f"xconv_3x3_{ci}to{co}_res{n}", ci, co, nres=n)
         for ci in (32, 48, 64, 80, 96, 128, 192) for co in (32, 48, 64, 96) for n in (0, 1, 2)]
BASE += [
    C("xconv_rw1_64to64_res1", 64, 64, nres=1, act=0.1),
    C("xconv_shuffle_64to64", 64, 64, shuf=True),
    C("xconv_7x7_8to32", 8, 32, 7),
    C("xconv_7x7_16to16", 16, 16, 7),
    C("xconv_7x7_32to32", 32, 32, 7),
    C("xconv_7x7_64to16", 64, 16, 7),
    C("dconv_3x3s2_64to64", 64, 64, 3, 2),
    C("dconv_3x3s2_128to96", 128, 96, 3, 2),
    C("dconv_3x3s2_64to96", 64, 96, 3, 2),
    C("dconv_1x1s2_64to64", 64, 64, 1, 2),
    C("dconv_1x1_64to128_shuffle_256x256", 64, 128, 1, 1, 256, 256, shuf=True),
    C("dconv_1x1_64to256_256x256", 64, 256, 1, 1, 256, 256),
    C("dconv_gated_1x1_64to64_256x256", 64, 64, 1, 1, 256, 256, gate=True, nres=1),
    C("dconv_1x1_64to128_shuffle_255x256", 64, 128, 1, 1, 255, 256, shuf=True),
    C("dconv_1x1_64to256_255x256", 64, 256, 1, 1, 255, 256),
    C("dconv_gated_1x1_64to64_255x256", 64, 64, 1, 1, 255, 256, gate=True, nres=1),
    C("sgemm_1x1_64to64", 64, 64, 1),
    C("sgemm_gated_1x1_64to64", 64, 64, 1, gate=True, nres=1),
    C("sconv_3x3_48to3", 48, 3),
    C("split_7x7s2_8to32_refused", 8, 32, 7, 2),
    C("split_7x7_8to32", 8, 32, 7, act=0.1),
    C("split_3x3_40to64", 40, 64),
    C("split_3x3_24to48", 24, 48),
    C("split_1x1_40to64", 40, 64, 1),
    C("split_1x1_24to48", 24, 48, 1),
    C("split_3x3s2_40to64", 40, 64, 3, 2),
    C("split_3x3s2_24to48", 24, 48, 3, 2),
]

# ---- the views and slopes a launcher refuses, on one layer of every family
FAMILY = [
    ("tconv", dict(cin=2, cout=64)),
    ("nconv", dict(cin=16, cout=2, k=7)),
    ("xconv", dict(cin=64, cout=64)),
    ("wconv", dict(cin=64, cout=64, opts={"wconv": 1})),
    ("dconv_s2", dict(cin=64, cout=64, s=2)),
    ("dconv_1x1", dict(cin=64, cout=64, k=1, H=256, W=256)),
    ("sgemm", dict(cin=64, cout=64, k=1)),
    ("sconv", dict(cin=48, cout=4)),
]
EDGE = [
    ("x_coff2", dict(xoff=2)),
    ("y_cstride_mod4", dict(ypad=2)),
    ("res_coff2", dict(nres=1, roff=2)),
    ("res2_without_res", dict(res2_only=True)),
    ("slope_1p5", dict(act=1.5)),
    ("in_slope_neg", dict(in_slope=-0.1)),
    ("bf16_y", dict(ydt="bf16")),
]
EDGES = [C(f"edge_{f}_{e}", **{**fk, **ek}) for f, fk in FAMILY for e, ek in EDGE]

# ---- each family's enable option switched
OPTS = [
    C("opt_xconv0", 64, 64, opts={"xconv": 0}),
    C("opt_dconv0", 64, 64, 3, 2, opts={"dconv": 0}),
    C("opt_dconv_1x1_0", 64, 256, 1, 1, 256, 256, opts={"dconv_1x1": 0}),
    C("opt_dconv_gate0", 64, 64, 1, 1, 256, 256, gate=True, nres=1, opts={"dconv_gate": 0}),
    C("opt_tconv0", 2, 64, opts={"tconv": 0}),
    C("opt_nconv0", 16, 2, 7, opts={"nconv": 0}),
    C("opt_sgemm_m1", 64, 64, 1, opts={"sgemm": -1}),
    C("opt_wconv1_64to64", 64, 64, opts={"wconv": 1}),
    C("opt_wconv1_128to128_res1", 128, 128, nres=1, opts={"wconv": 1}),
]

# ---- bf16 and fp32 compute: the dispatcher branches of dcvc_conv2d
_B = dict(compute="bf16", dt="bf16")
_F = dict(compute="f32")
OTHER = [
    C("bf16_3x3_64to64", 64, 64, **_B),
    C("bf16_3x3_64to64_272x480", 64, 64, 3, 1, 272, 480, **_B),
    C("bf16_1x1_64to64", 64, 64, 1, **_B),
    C("bf16_1x1_128to128_272x480", 128, 128, 1, 1, 272, 480, **_B),
    C("bf16_3x3s2_64to64", 64, 64, 3, 2, **_B),
    C("bf16_3x3s2_64to64_544x960", 64, 64, 3, 2, 544, 960, **_B),
    C("bf16_7x7_8to32", 8, 32, 7, **_B),
    C("bf16_7x7_32to32", 32, 32, 7, **_B),
    C("bf16_7x7_8to32_272x480", 8, 32, 7, 1, 272, 480, **_B),
    C("bf16_7x7_32to32_272x480", 32, 32, 7, 1, 272, 480, **_B),
    C("f32_1x1_64to64", 64, 64, 1, **_F),
    C("f32_3x3_64to64", 64, 64, 3, **_F),
    C("bf16_generic_5x5_24to40", 24, 40, 5, **_B),
    C("bf16_compute_f32_views_3x3_64to64", 64, 64, compute="bf16"),
    C("f32_generic_5x5_24to40", 24, 40, 5, **_F),
]

CASES = BASE + EDGES + OPTS + OTHER
assert len({c["name"] for c in CASES}) == len(CASES)

_recorded = {}


def route(c):
    """The kernel the call launched, or "error: ..." for a call that raised."""
    h = K()
    from dcvc_amd._native import NativeError
    comp = {"f16x3": h.F16X3, "bf16": h.BF16, "f32": h.F32}[c.get("compute", "f16x3")]
    dt = {"f32": h.F32, "bf16": h.BF16}[c.get("dt", "f32")]
    ydt = {"f32": h.F32, "bf16": h.BF16, None: dt}[c.get("ydt")]
    cin, cout, k, s, H, W = c["cin"], c["cout"], c["k"], c["s"], c["H"], c["W"]
    shuf, gate = c.get("shuf", False), c.get("gate", False)
    g = torch.Generator().manual_seed(1)
    cw = h.ConvW(torch.randn(cout, cin, k, k, generator=g) * 0.05, torch.zeros(cout), s, comp)
    cx = 2 * cin if gate else cin
    xoff = c.get("xoff", 0)
    x = h.zeros(H, W, cx + 2 * xoff, dt).ch(xoff, cx)
    Ho, Wo = cw.out_hw(H, W)
    f = 2 if shuf else 1
    cy = cout // 4 if shuf else cout
    y = h.zeros(Ho * f, Wo * f, cy + c.get("ypad", 0), ydt).ch(0, cy)
    roff = c.get("roff", 0)
    rs = [h.zeros(Ho * f, Wo * f, cy + 2 * roff, ydt).ch(roff, cy) for _ in range(c.get("nres", 0))]
    res = rs[0] if rs else None
    res2 = rs[1] if len(rs) > 1 else None
    if c.get("res2_only"):
        res, res2 = None, h.zeros(Ho * f, Wo * f, cy, ydt)
    act = c.get("act")
    in_slope = c.get("in_slope")
    kw = dict(act=h.ACT_NONE if act is None else h.ACT_LRELU, slope=act or 0.0, shuffle=shuf, res=res, res2=res2,
              in_op=h.IN_GATE if gate else h.IN_NONE if in_slope is None else h.IN_LRELU,
              in_slope=0.1 if gate else in_slope or 0.0)
    opts = c.get("opts", {})
    saved = {n: h.get_option(n) for n in opts}
    try:
        for n, v in opts.items():
            h.set_option(n, v)
        try:
            h.conv(cw, x, y, **kw)
            torch.cuda.synchronize()
            return h.lib().dcvc_last_kernel().decode()
        except NativeError as e:
            return f"error: {e}"
    finally:
        for n, v in saved.items():
            h.set_option(n, v)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_conv_routing(c):
    from dcvc_amd._native import _ERRORS
    got = route(c)
    # a refusal (invalid / unsupported) is a route like any other, a failed launch
    # (DCVC_HIP_ELAUNCH = -2, in check()'s words) never is, on any library
    assert got and got != f"error: conv2d: {_ERRORS[-2]}", got
    if RECORD:
        _recorded[c["name"]] = got
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert got == golden[c["name"]]


def test_golden_has_one_entry_per_case():
    if RECORD:
        assert sorted(_recorded) == sorted(c["name"] for c in CASES)
        with open(GOLDEN, "w") as f:
            json.dump(_recorded, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(c["name"] for c in CASES)

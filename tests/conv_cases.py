"""The dcvc_conv2d calls the suite pins, as one table with two readers.

tests/test_gpu_conv_routing.py records which kernel takes each call (on
all-zero tensors: a route must not depend on data), and
tests/test_gpu_conv_conformance.py makes the same calls on random data and
compares the values with reference() below: an fp64 restatement of the formula
include/dcvc_hip.h gives for dcvc_conv_args,

    y = scale[c] * (res2 + (res + act(conv(in_op(x)) + bias)))   (+ pixel shuffle)

written from the header's definitions (the selects of dcvc_act / dcvc_in_op),
never from a kernel.  tests/test_conv_cases.py checks reference() itself
against a straight-line torch composition, without a GPU.

build(c, "zeros") is the call of the routing test; build(c, "random") is the
same call (same views, same options, plus a per-channel scale where the case
does not forbid it) on the data of tensors(c).  Nothing here needs a GPU
except build() and launch().
"""
import json
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routing.json")
SENTINEL = 7.0   # build(c, "random") fills the whole output buffer with it


def C(name, cin, cout, k=3, s=1, H=32, W=48, **kw):
    """One case.  Keywords: compute ("f16x3" | "bf16" | "f32"), dt (dtype of
    the views: "f32" | "bf16"), ydt (of y alone), nres, shuf, gate, act slope
    `act` (None: no activation), epi ("clamp01" | "round": that activation
    instead of the leaky ReLU, `act` still passed as the slope argument),
    input leaky ReLU slope `in_slope` (with gate: the gate's slope, 0.1 when
    absent), xoff (input window offset in a wider buffer), ypad (extra
    channels of the output buffer), roff (residual window offset), res2_only,
    opts, noscale (random data: no per-channel scale)."""
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
# the slopes at and beyond the edge of the max form max(v, s * v) the split
# kernels compute (exact for s <= 1 only), the ReLU the models pass as slope 0,
# and the two activations no family test reaches
EDGE += [
    ("in_slope_1p5", dict(in_slope=1.5)),
    ("in_slope_1", dict(in_slope=1.0)),
    ("slope_0", dict(act=0.0)),
    ("slope_1", dict(act=1.0)),
    ("act_clamp01", dict(epi="clamp01")),
    ("act_round", dict(epi="round")),
]
EDGES = [C(f"edge_{f}_{e}", **{**fk, **ek}) for f, fk in FAMILY for e, ek in EDGE]
EDGES += [C(f"edge_{f}_gate_in_slope_1p5", **{**fk, **dict(gate=True, nres=1, in_slope=1.5)})
          for f, fk in FAMILY if f in ("dconv_1x1", "sgemm")]

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

# ---- the models' clamping and rounding layers, with the kernel size, stride
# and channel counts of dcvc_amd/data/dc_param_spec.json / hem_param_spec.json:
# the reconstruction convs (*.recon_conv 48 -> 3 and 64 -> 3, refine.1 16 -> 3:
# clamp to [0, 1], fp32 output, from fp32 and from bf16 features) and the hyper
# encoders' last conv (3x3 stride 2, 64 / 128 / 192 wide: round, called with
# slope 0.01 as layers.py hyper_enc passes it)
_BF = dict(compute="bf16", dt="bf16", ydt="f32")
MODEL = [
    C("model_dc_recon_conv_48to3_clamp", 48, 3, epi="clamp01"),
    C("model_dc_recon_conv_48to3_clamp_bf16", 48, 3, epi="clamp01", **_BF),
    C("model_dc_recon_conv_48to3_clamp_f32", 48, 3, epi="clamp01", **_F),
    C("model_hem_recon_conv_64to3_clamp", 64, 3, epi="clamp01"),
    C("model_hem_recon_conv_64to3_clamp_bf16", 64, 3, epi="clamp01", **_BF),
    C("model_refine1_16to3_clamp", 16, 3, epi="clamp01"),
    C("model_refine1_16to3_clamp_bf16", 16, 3, epi="clamp01", **_BF),
    C("model_mv_henc8_3x3s2_64to64_round", 64, 64, 3, 2, epi="round", act=0.01),
    C("model_mv_henc8_3x3s2_64to64_round_f32", 64, 64, 3, 2, epi="round", act=0.01, **_F),
    C("model_dc_y_henc4_3x3s2_128to128_round", 128, 128, 3, 2, epi="round", act=0.01),
    C("model_hem_henc8_3x3s2_192to192_round", 192, 192, 3, 2, epi="round", act=0.01),
]

CASES = BASE + EDGES + OPTS + OTHER + MODEL
assert len({c["name"] for c in CASES}) == len(CASES)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def compute_of(c):
    return c.get("compute", "f16x3")


def f32(v):
    """A Python float as the C ABI's float argument carries it."""
    return float(np.float32(v))


def geometry(c):
    """Sizes of the call's buffers and views: what route() of the routing
    test derived inline."""
    cin, cout, k, s, H, W = c["cin"], c["cout"], c["k"], c["s"], c["H"], c["W"]
    shuf, gate = c.get("shuf", False), c.get("gate", False)
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    f = 2 if shuf else 1
    nres = c.get("nres", 0)
    return dict(cx=2 * cin if gate else cin, xoff=c.get("xoff", 0), pad=pad, Ho=Ho, Wo=Wo, Hy=Ho * f, Wy=Wo * f,
                cy=cout // 4 if shuf else cout, ypad=c.get("ypad", 0), roff=c.get("roff", 0),
                res=nres > 0 and not c.get("res2_only"), res2=nres > 1 or bool(c.get("res2_only")),
                r2off=0 if c.get("res2_only") else c.get("roff", 0))


def _tdt(name):
    return {"f32": torch.float32, "bf16": torch.bfloat16}[name]


def _in_op(c, x, slope):
    """in_op(x) of dcvc_in_op on an NCHW tensor, in x's own precision: the
    select v >= 0 ? v : v * in_slope, and for the gate x[c] * lrelu(x[c + Cin])."""
    def lrelu(v):
        return torch.where(v >= 0, v, v * slope)
    if c.get("gate"):
        return x[:, :c["cin"]] * lrelu(x[:, c["cin"]:])
    if c.get("in_slope") is not None:
        return lrelu(x)
    return x


def _conv64(t, w, s, pad, rows=64):
    """F.conv2d in fp64, in strips of output rows (the im2col buffer of the
    largest maps stays small)."""
    Ho = (t.shape[2] + 2 * pad - w.shape[2]) // s + 1
    if Ho <= rows:
        return F.conv2d(t, w, stride=s, padding=pad)
    t = F.pad(t, (pad, pad, pad, pad))
    k = w.shape[2]
    return torch.cat([F.conv2d(t[:, :, r * s:(min(r + rows, Ho) - 1) * s + k], w, stride=s)
                      for r in range(0, Ho, rows)], 2)


def _nchw(hwc):
    return hwc.permute(2, 0, 1).unsqueeze(0)


def preact(c, t):
    """conv(in_op(x)) + bias in fp64, (1, cout, Ho, Wo): the value the
    activation sees.  bf16 compute: of the operands as the kernels stage them
    (the input op in fp32, then x and w rounded to bf16)."""
    g = geometry(c)
    x = _nchw(t["x"][:, :, g["xoff"]:g["xoff"] + g["cx"]])
    if c.get("gate"):
        slope = f32(c.get("in_slope", 0.1))
    else:
        slope = f32(c.get("in_slope") or 0.0)
    if compute_of(c) == "bf16":
        xin = _in_op(c, x.float(), slope).bfloat16().double()
        w = t["w"].bfloat16().double()
    else:
        xin = _in_op(c, x.double(), slope)
        w = t["w"].double()
    return _conv64(xin, w, c["s"], g["pad"]) + t["bias"].double().view(1, -1, 1, 1)


def reference(c, t, pre=None):
    """The ABI's formula in fp64 on the tensors of tensors(c): (Hy, Wy, cy),
    the layout of the y view."""
    g = geometry(c)
    v = preact(c, t) if pre is None else pre
    slope = f32(c.get("act") or 0.0)
    if c.get("epi") == "clamp01":
        v = torch.clamp(torch.clamp(v, min=0.0), max=1.0)
    elif c.get("epi") == "round":
        v = torch.round(v)                  # half to even
    elif c.get("act") is not None:
        v = torch.where(v >= 0, v, v * slope)
    if c.get("shuf"):
        v = F.pixel_shuffle(v, 2)
    v = v[0].permute(1, 2, 0)
    if t["res"] is not None:
        v = t["res"][:, :, g["roff"]:g["roff"] + g["cy"]].double() + v
    if t["res2"] is not None:
        v = t["res2"][:, :, g["r2off"]:g["r2off"] + g["cy"]].double() + v
    if t["scale"] is not None:
        v = v * t["scale"].double()         # indexed by the channel of y (after the shuffle)
    return v


def clamp_shares(pre):
    """Of a clamp01 case's pre-activation: the shares of elements that
    saturate at 0, saturate at 1, and lie strictly inside."""
    lo, hi = (pre <= 0).double().mean().item(), (pre >= 1).double().mean().item()
    return lo, hi, 1.0 - lo - hi


def round_band(c_bound, pre):
    """Of a round case's pre-round values: the mask of elements within
    c_bound * max|pre| of a half-integer, which may round either way within
    the compute mode's bound."""
    return (pre - torch.floor(pre) - 0.5).abs() <= c_bound * pre.abs().max().item()


def tensors(c):
    """The random data of a case, on the CPU, from a generator seeded by the
    case's name (see _draw).  A clamp01 case takes the first of its draws that
    saturates 2.5 % of the elements on each side: the rescaling goes by max|v|,
    the one extreme value of the draw, and on the thin and the large layers
    (2 -> 64, 256 x 256) one draw in three stays below the 2 % the tests ask
    of the data."""
    if c.get("epi") != "clamp01":
        return _draw(c, 0)
    for salt in range(16):
        t = _draw(c, salt)
        lo, hi, inside = clamp_shares(preact(c, t))
        if min(lo, hi) >= 0.025 and inside >= 0.5:
            return t
    raise AssertionError(c["name"])


def _draw(c, salt):
    """Draw `salt` of a case's data, from a generator seeded by its name: x (H, W, buffer channels; randn, every third row * 1e-3 so
    the fp16 lo parts of the split go subnormal; the channels around an offset
    view are random too), w (randn / sqrt(cin k k)), bias (randn * 0.1), res /
    res2 (whole buffers, randn), scale (rand + 0.5, None where the case
    forbids it).  bf16 views hold bf16 values.

    clamp01 cases: w and bias are rescaled so that the pre-activation v becomes
    0.5 + 1.5 v / max|v|: both clamps act and most values lie inside.
    round cases: x is scaled by 4 (outputs span about +-20 integers) and no
    scale is applied (the integers are compared exactly)."""
    g = geometry(c)
    gen = torch.Generator().manual_seed(zlib.crc32(c["name"].encode() + b"." * salt))
    cin, cout, k, H, W = c["cin"], c["cout"], c["k"], c["H"], c["W"]
    dt = _tdt(c.get("dt", "f32"))
    ydt = _tdt(c.get("ydt") or c.get("dt", "f32"))
    x = torch.randn(g["cx"] + 2 * g["xoff"], H, W, generator=gen)
    x[:, ::3] *= 1e-3
    if c.get("epi") == "round":
        x *= 4.0
    x = x.permute(1, 2, 0).contiguous().to(dt)
    w = torch.randn(cout, cin, k, k, generator=gen) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=gen) * 0.1

    def resbuf(on, off):
        if not on:
            return None
        return torch.randn(g["Hy"], g["Wy"], g["cy"] + 2 * off, generator=gen).to(ydt)
    res = resbuf(g["res"], g["roff"])
    res2 = resbuf(g["res2"], g["r2off"])
    scale = None
    if not c.get("noscale") and c.get("epi") != "round":
        scale = torch.rand(g["cy"], generator=gen) + 0.5
    t = dict(x=x, w=w, bias=bias, res=res, res2=res2, scale=scale)
    if c.get("epi") == "clamp01":
        m = 1.5 / preact(c, t).abs().max().item()
        t["w"] = (w.double() * m).float()
        t["bias"] = (0.5 + bias.double() * m).float()
    return t


def build(c, data):
    """The call of case c on the GPU: (cw, x, y, kwargs, buffers) for
    hip.conv(cw, x, y, **kwargs).  data = "zeros": all-zero views, zero bias,
    no scale (the routing test's call).  data = "random": the same views on
    the data of tensors(c), a scale where that has one, and the whole output
    buffer filled with SENTINEL.  buffers: the CPU tensors of tensors(c) (None
    for zeros) and "ybuf", the Act of the whole output buffer.  launch()
    sets the case's options (c["opts"]) around the call."""
    from dcvc_amd import hip as h
    assert data in ("zeros", "random")
    rnd = data == "random"
    g = geometry(c)
    comp = {"f16x3": h.F16X3, "bf16": h.BF16, "f32": h.F32}[compute_of(c)]
    dt = {"f32": h.F32, "bf16": h.BF16}[c.get("dt", "f32")]
    ydt = {"f32": h.F32, "bf16": h.BF16, None: dt}[c.get("ydt")]
    cin, cout, k, s, H, W = c["cin"], c["cout"], c["k"], c["s"], c["H"], c["W"]
    shuf, gate = c.get("shuf", False), c.get("gate", False)
    Hy, Wy, cy = g["Hy"], g["Wy"], g["cy"]
    t = tensors(c) if rnd else None

    def up(a):
        return h.Act(a.cuda())

    if rnd:
        cw = h.ConvW(t["w"], t["bias"], s, comp)
        xb = up(t["x"])
        yb = h.zeros(Hy, Wy, cy + g["ypad"], ydt)
        yb.buf.fill_(SENTINEL)
    else:
        gen = torch.Generator().manual_seed(1)
        cw = h.ConvW(torch.randn(cout, cin, k, k, generator=gen) * 0.05, torch.zeros(cout), s, comp)
        xb = h.zeros(H, W, g["cx"] + 2 * g["xoff"], dt)
        yb = h.zeros(Hy, Wy, cy + g["ypad"], ydt)
    assert cw.out_hw(H, W) == (g["Ho"], g["Wo"])
    x = xb.ch(g["xoff"], g["cx"])
    y = yb.ch(0, cy)

    def resview(name, on, off):
        if not on:
            return None
        b = up(t[name]) if rnd else h.zeros(Hy, Wy, cy + 2 * off, ydt)
        return b.ch(off, cy)
    res = resview("res", g["res"], g["roff"])
    res2 = resview("res2", g["res2"], g["r2off"])
    act, epi, in_slope = c.get("act"), c.get("epi"), c.get("in_slope")
    kw = dict(act={"clamp01": h.ACT_CLAMP01, "round": h.ACT_ROUND}[epi] if epi
              else h.ACT_NONE if act is None else h.ACT_LRELU,
              slope=act or 0.0, shuffle=shuf, res=res, res2=res2,
              in_op=h.IN_GATE if gate else h.IN_NONE if in_slope is None else h.IN_LRELU,
              in_slope=(0.1 if in_slope is None else in_slope) if gate else in_slope or 0.0)
    if rnd and t["scale"] is not None:
        kw["scale"] = t["scale"].cuda()
    buffers = dict(t or {}, ybuf=yb)
    return cw, x, y, kw, buffers


def launch(c, data):
    """build(c, data) and the call, under the case's options: (the kernel it
    launched, as dcvc_last_kernel() spells it, or "error: ..." for a call
    that raised; buffers)."""
    from dcvc_amd import hip as h
    from dcvc_amd._native import NativeError
    cw, x, y, kw, buffers = build(c, data)
    opts = c.get("opts", {})
    saved = {n: h.get_option(n) for n in opts}
    try:
        for n, v in opts.items():
            h.set_option(n, v)
        try:
            h.conv(cw, x, y, **kw)
            torch.cuda.synchronize()
            return h.lib().dcvc_last_kernel().decode(), buffers
        except NativeError as e:
            return f"error: {e}", buffers
    finally:
        for n, v in saved.items():
            h.set_option(n, v)

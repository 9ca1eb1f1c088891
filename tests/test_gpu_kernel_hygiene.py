"""Kernel hygiene: no kernel's output may depend on memory outside its views.

One table entry per kernel route of the default (split) path and of the
helper kernels the models and the harness call.  Every entry builds its call
through tests/hygiene.py, so each Act argument is a channel window of a wider
buffer with guard rows above and below, each raw pointer a slice of a guarded
1-D allocation.  Per entry (hygiene.run_entry):

  1. the clean run against an fp64 (or exact integer) restatement of the
     operation on the view alone, at the tolerance of the family's own test
     file (cited beside each entry);
  2. with every input's surroundings NaN and 1e30: the outputs bit-identical
     to the clean run (two clean runs are compared first);
  3. routes that feed the split range guard: armed, it must not trip on the
     1e30 around the views;
  4. nothing stored outside any view, no output element left unwritten;
  5. after dcvc_debug_poison_lds / dcvc_debug_poison_vgpr on the stream: the
     same bits again.

Shapes are the ragged cases of the families' own tests: a partial last tile in
both directions, a channel tail, more than one tile or block.

test_every_launcher_has_a_hygiene_case (CPU) walks hip.HIP_SYMBOLS: a launcher
with a tensor argument must be named by a table entry or by EXCLUDED.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcvc_amd import hip as K
from tests import entropy_ref as R
from tests import hygiene as HY
from tests.hygiene import LEAD, seeded

gpu = pytest.mark.gpu

TOL_SPLIT = 4e-6     # TOL of test_gpu_xconv.py, test_gpu_sconv.py, test_gpu_dconv.py, test_gpu_tconv.py, test_gpu_nconv.py
TOL_DW = 1e-5        # test_gpu_kernels.py test_dwconv3x3 (rel_err)
TOL_OD = 1e-4        # test_gpu_kernels.py test_offset_diversity_matches_oracle (absolute)
TOL_RESAMPLE = 1e-6  # test_gpu_kernels.py test_resize_and_pool (absolute)
TOL_SE = 1e-5        # test_gpu_kernels.py test_se_layer_matches_torch (scale absolute, f32 apply rel_err)
TOL_SSE = 1e-12      # test_harness.py test_frame_sse_and_inplace_clamp (rtol)
TOL_SSIM = 1e-10     # test_harness.py test_gpu_msssim_matches_reference_fixtures (absolute)
BITS_REL = 1e-5      # test_gpu_entropy_kernels.py BITS_REL

SCONV_ONLY = {"xconv": 0, "dconv": 0, "tconv": 0, "nconv": 0}   # the fixture of test_gpu_sconv.py


@contextlib.contextmanager
def options(opts):
    old = {k: K.get_option(k) for k in opts or {}}
    for k, v in (opts or {}).items():
        K.set_option(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            K.set_option(k, v)


def want_route(E, *prefixes, contains=None):
    """The last launch took the kernel the entry is about (a dry run launches nothing)."""
    if E.dry:
        return
    r = E.routes[-1]
    assert r.startswith(prefixes), (r, prefixes)
    assert contains is None or contains in r, (r, contains)


def small_rows(x):
    x = x.clone()
    x[:, :, ::3] *= 1e-3          # small values: the lo parts go subnormal in fp16 (test_gpu_xconv.py)
    return x


# name -> (fn, symbols, guard, deterministic)
TABLE = {}


def entry(name, *symbols, guard=False, deterministic=True):
    def deco(fn):
        assert name not in TABLE
        TABLE[name] = (fn, symbols, guard, deterministic)
        return fn
    return deco


# ------------------------------------------------------------------- dcvc_conv2d
def conv_case(E, cin, cout, k, s, H, W, want, lrelu=False, act=False, nres=0, scaled=False, shuf=False,
              gate=False, opts=None, lead=LEAD, ylead=LEAD, ytail=LEAD, contains=None):
    """out = scale * (res2 + (res + act(conv(in_op(x)) + bias))) in split precision."""
    xc = 2 * cin if gate else cin
    x = E.const("x", lambda: small_rows(torch.randn(1, xc, H, W, generator=seeded("x"))))
    w = E.randn("w", cout, cin, k, k, scale=1.0 / (cin * k * k) ** 0.5)
    b = E.randn("b", cout, scale=0.1)
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    co, f = (cout // 4, 2) if shuf else (cout, 1)
    rs = [E.randn(f"r{i}", 1, co, Ho * f, Wo * f) for i in range(nres)]
    sc = E.const("sc", lambda: torch.rand(co, generator=seeded("sc")) + 0.5) if scaled else None
    cw = E.const("cw", lambda: K.ConvW(w, b, s, K.F16X3, device=E.dev))
    xa = E.x(x, lead=lead)
    ra = [E.x(r) for r in rs]
    y = E.y("y", co, Ho * f, Wo * f, lead=ylead, tail=ytail)
    in_slope = 0.1 if gate else 0.01
    kw = dict(act=K.ACT_LRELU if act else K.ACT_NONE, slope=0.1, shuffle=shuf,
              scale=E.dev_const("sc", lambda: sc) if scaled else None,
              in_op=K.IN_GATE if gate else (K.IN_LRELU if lrelu else K.IN_NONE), in_slope=in_slope,
              res=ra[0] if nres > 0 else None, res2=ra[1] if nres > 1 else None)
    with options(opts):
        E.launch(K.conv, cw, xa, y, **kw)
    want_route(E, *((want,) if isinstance(want, str) else want), contains=contains)

    def ref():
        xd = x.double()
        if gate:
            xd = xd[:, :cin] * F.leaky_relu(xd[:, cin:], in_slope)
        elif lrelu:
            xd = F.leaky_relu(xd, in_slope)
        r = F.conv2d(xd, w.double(), b.double(), stride=s, padding=pad)
        if act:
            r = F.leaky_relu(r, 0.1)
        if shuf:
            r = F.pixel_shuffle(r, 2)
        for t in rs:
            r = t.double() + r
        return r * sc.double().view(1, -1, 1, 1) if scaled else r
    E.ref("y", ref, TOL_SPLIT)


def conv_entry(name, *a, **kw):
    entry(name, "dcvc_conv2d", guard=True)(lambda E: conv_case(E, *a, **kw))


# static-shape 3x3 / 7x7 (xconv.hip; CASES, SHUF_CASES, K7_CASES of test_gpu_xconv.py)
conv_entry("xconv3 48->48 37x53 lrelu-in 2 residuals", 48, 48, 3, 1, 37, 53, "xconv3_kernel", lrelu=True, act=True,
           nres=2, scaled=True)
# more tiles (17 x 34 = 578) than the persistent grid has workgroups (2 per CU): the weight ring and the
# image double buffer carry over from tile to tile (P3_CASES' 261x533 of test_gpu_kernels.py)
conv_entry("xconv3 48->48 261x533 several tiles per workgroup", 48, 48, 3, 1, 261, 533, "xconv3_kernel", lrelu=True,
           act=True, nres=1)
conv_entry("xconv3 80->48 40x66", 80, 48, 3, 1, 40, 66, "xconv3_kernel", act=True, scaled=True)
conv_entry("xconv3 128->32 19x23", 128, 32, 3, 1, 19, 23, "xconv3_kernel", act=True)
conv_entry("xconv3 shuffle 32->80 19x21", 32, 80, 3, 1, 19, 21, "xconv3_kernel", act=True, shuf=True)
conv_entry("xconv3 7x7 8->32 36x70", 8, 32, 7, 1, 36, 70, "xconv3_kernel", act=True)
# thin fp32-VALU convs on 2-channel inputs (tconv.hip; CASES of test_gpu_tconv.py)
conv_entry("tconv 2->64 3x3 s2 37x51", 2, 64, 3, 2, 37, 51, "tconv_", lrelu=True, act=True, nres=1, scaled=True,
           lead=4)
conv_entry("tconv 2->128 1x1 s2 17x30", 2, 128, 1, 2, 17, 30, "tconv_", lead=4)
# few-output-channel 7x7 (nconv.hip; CASES of test_gpu_nconv.py)
conv_entry("nconv 16->2 7x7 16x16", 16, 2, 7, 1, 16, 16, "nconv_kernel", lead=4, ylead=2, ytail=3)
# direct split conv (dconv.hip; CASES and the gated cases of test_gpu_dconv.py)
conv_entry("dconv 56->64 3x3 s2 37x53", 56, 64, 3, 2, 37, 53, "dconv_kernel", lead=4, ylead=4)
conv_entry("dconv 64->64 1x1 s2 68x122", 64, 64, 1, 2, 68, 122, "dconv_kernel", lead=4, ylead=4)
conv_entry("dconv 64->256 1x1 shuffle 256x260", 64, 256, 1, 1, 256, 260, "dconv_kernel<1", shuf=True, scaled=True,
           lead=4, ylead=4)
conv_entry("dconv gated 64->16 1x1 260x256", 64, 16, 1, 1, 260, 256, "dconv_kernel<1", gate=True, nres=1,
           contains=", true>")
# pixel GEMM (sgemm.hip; test_sgemm_matches_fp64 and test_sgemm_gated_1x1_matches_sconv)
conv_entry("sgemm 192->48 9x7", 192, 48, 1, 1, 9, 7, "sgemm_kernel", lead=4, ylead=4)
conv_entry("sgemm gated 96->40 17x23", 96, 40, 1, 1, 17, 23, "sgemm_kernel", gate=True, nres=1, contains=", true>")
# generic split conv (sconv.hip; CASES of test_gpu_sconv.py, routed as its fixture does)
conv_entry("sconv 51->64 3x3 s2 34x40", 51, 64, 3, 2, 34, 40, "sconv_kernel", opts=SCONV_ONLY)
conv_entry("sconv 3->48 3x3 20x33", 3, 48, 3, 1, 20, 33, "sconv_kernel", opts=SCONV_ONLY, act=True)
conv_entry("sconv 16->2 7x7 16x16", 16, 2, 7, 1, 16, 16, "sconv_kernel", opts=SCONV_ONLY)
# views at channel offset 2: the scalar staging / element-store paths
conv_entry("conv 48->48 3x3 37x53 at offset 2", 48, 48, 3, 1, 37, 53, ("sconv_kernel", "xconv3_kernel"), lrelu=True,
           act=True, nres=1, lead=2, ylead=2)
conv_entry("conv 192->48 1x1 9x7 at offset 2", 192, 48, 1, 1, 9, 7, ("sconv_kernel", "sgemm_kernel"), lead=2, ylead=2)


# ------------------------------------------------------- fused split blocks
def ffn_case(E, c, H, W, want, lead=4):
    """ConvFFN (test_fused_ffn_matches_fp64 / test_latent_ffn_matches_fp64_and_unfused)."""
    hid = 4 * c if c <= 128 else max(min(4 * c, 1024), 2 * c)
    x = E.randn("x", 1, c, H, W)
    w1, b1 = E.randn("w1", hid, c, 1, 1, scale=c ** -0.5), E.randn("b1", hid, scale=0.1)
    w2, b2 = E.randn("w2", c, hid, 1, 1, scale=hid ** -0.5), E.randn("b2", c, scale=0.1)
    sc = E.const("sc", lambda: torch.rand(c, generator=seeded("sc")) + 0.5)
    fw = E.const("fw", lambda: K.FfnW(w1, b1, w2, b2, device=E.dev))
    xa, y = E.x(x, lead=lead), E.y("y", c, H, W, lead=lead)
    r = E.launch(K.conv_ffn, fw, xa, y, scale=E.dev_const("sc", lambda: sc), slope=0.1)
    assert E.dry or r is not None
    want_route(E, want)

    def ref():
        xd = x.double()
        hh = F.leaky_relu(F.conv2d(xd, w1.double(), b1.double()), 0.1)
        return (xd + F.leaky_relu(F.conv2d(hh, w2.double(), b2.double()), 0.1)) * sc.double().view(1, -1, 1, 1)
    E.ref("y", ref, TOL_SPLIT)


entry("conv_ffn sffn 48 37x53", "dcvc_conv_ffn", guard=True)(lambda E: ffn_case(E, 48, 37, 53, "sffn_kernel"))
# 259 pixel tiles for 256 persistent workgroups (the 200x331 map of test_fused_ffn_matches_fp64)
entry("conv_ffn sffn 48 200x331 several tiles per workgroup", "dcvc_conv_ffn", guard=True)(
    lambda E: ffn_case(E, 48, 200, 331, "sffn_kernel"))
entry("conv_ffn slffn 192 5x7", "dcvc_conv_ffn", guard=True)(lambda E: ffn_case(E, 192, 5, 7, "slffn_kernel"))
entry("conv_ffn slffn 384 3x11", "dcvc_conv_ffn", guard=True)(lambda E: ffn_case(E, 384, 3, 11, "slffn_kernel"))


def dwc_case(E, c, H, W):
    """The tail of a latent DepthConv (test_latent_dw_conv2_matches_fp64_and_unfused)."""
    t, x = E.randn("t", 1, c, H, W), E.randn("x", 1, c, H, W)
    wd, bd = E.randn("wd", c, 1, 3, 3, scale=1 / 3), E.randn("bd", c, scale=0.1)
    w2, b2 = E.randn("w2", c, c, 1, 1, scale=c ** -0.5), E.randn("b2", c, scale=0.1)
    dwc = E.const("dwc", lambda: K.DwcW(wd.reshape(c, 9).t().contiguous(), bd, w2, b2, device=E.dev))
    ta, xa, y = E.x(t), E.x(x, lead=4), E.y("y", c, H, W, lead=4)
    r = E.launch(K.dw_conv2_split, dwc, ta, xa, y)
    assert E.dry or r is not None
    want_route(E, "sldc_kernel")
    E.ref("y", lambda: F.conv2d(F.conv2d(t.double(), wd.double(), bd.double(), padding=1, groups=c), w2.double(),
                                b2.double()) + x.double(), TOL_SPLIT)


entry("dw_conv2_split 192 5x7", "dcvc_dw_conv2_split", guard=True)(lambda E: dwc_case(E, 192, 5, 7))
entry("dw_conv2_split 384 1x40", "dcvc_dw_conv2_split", guard=True)(lambda E: dwc_case(E, 384, 1, 40))


@entry("depth_conv_split 48->32 adaptor 20x33", "dcvc_depth_conv_split", guard=True)
def _sdc(E, cin=48, cout=32, H=20, W=33):
    """Fused DepthConv (test_fused_depthconv_matches_fp64)."""
    x = E.randn("x", 1, cin, H, W)
    w1, b1 = E.randn("w1", cin, cin, 1, 1, scale=cin ** -0.5), E.randn("b1", cin, scale=0.1)
    wd, bd = E.randn("wd", cin, 1, 3, 3, scale=1 / 3), E.randn("bd", cin, scale=0.1)
    w2, b2 = E.randn("w2", cout, cin, 1, 1, scale=cin ** -0.5), E.randn("b2", cout, scale=0.1)
    wa, ba = E.randn("wa", cout, cin, 1, 1, scale=cin ** -0.5), E.randn("ba", cout, scale=0.1)
    dw = E.const("dw", lambda: K.DcW(w1, b1, wd.reshape(cin, 9).t().contiguous(), bd, w2, b2, wa, ba, device=E.dev))
    xa, y = E.x(x, lead=4), E.y("y", cout, H, W)
    r = E.launch(K.depth_conv_split, dw, xa, y, slope=0.01)
    assert E.dry or r is not None
    want_route(E, "sdc_kernel")

    def ref():
        xd = x.double()
        t = F.leaky_relu(F.conv2d(xd, w1.double(), b1.double()), 0.01)
        t = F.conv2d(t, wd.double(), bd.double(), padding=1, groups=cin)
        return F.conv2d(t, w2.double(), b2.double()) + F.conv2d(xd, wa.double(), ba.double())
    E.ref("y", ref, TOL_SPLIT)


@entry("depthconv_block bf16 48->32 37x45", "dcvc_depthconv_block")
def _dcb(E, cin=48, cout=32, H=37, W=45):
    """The fused bf16 DepthConvBlock of Precision.fast() (not on the split path;
    the fast models still call it) against the fp32 oracle on the bf16-rounded
    input: rel_err < 3e-2 as test_fused_depthconv_block_matches_unfused."""
    from dcvc_amd import layers as L
    from oracle import dc_oracle as O
    from tests.test_gpu_kernels import _dcb_state
    sd = E.const("sd", lambda: _dcb_state(cin, cout, False, seed=cin * 7 + cout))
    blk = E.const("blk", lambda: L.DepthConvBlock(L.Ctx(sd, E.dev, L.Precision.fast()), "b"))
    x = E.const("x", lambda: torch.randn(1, cin, H, W, generator=seeded("x")).bfloat16().float())
    sc = E.const("sc", lambda: torch.rand(cout, generator=seeded("sc")) + 0.5)
    xa, y = E.x(x, K.BF16), E.y("y", cout, H, W, K.BF16)
    r = E.launch(K.depthconv_block, blk, xa, y, E.dev_const("sc", lambda: sc))
    assert E.dry or r is not None
    want_route(E, "dcb")
    E.ref("y", lambda: O.depth_conv_block(O.Params(sd), "b", x).double() * sc.double().view(1, -1, 1, 1), 3e-2)


# 17 x 17 = 289 tiles of 8 x 16 pixels for 256 persistent workgroups
entry("depth_conv_split 48->32 adaptor 133x261 several tiles per workgroup", "dcvc_depth_conv_split", guard=True)(
    lambda E: _sdc(E, 48, 32, 133, 261))


def dw_case(E, C, H, W, lead):
    """Depthwise 3x3 (test_dwconv3x3_f32_row_blocked_bit_identical: aligned views
    take dw4r_kernel, offset 2 the scalar kernel)."""
    x, w, b = E.randn("x", 1, C, H, W), E.randn("w", C, 1, 3, 3), E.randn("b", C)
    w9c = E.dev_const("w9c", lambda: w.reshape(C, 9).t().contiguous())
    xa, y = E.x(x, lead=lead), E.y("y", C, H, W, lead=lead)
    E.launch(K.dwconv3x3, xa, w9c, E.dev_const("b", lambda: b), y=y)
    E.ref("y", lambda: F.conv2d(x.double(), w.double(), b.double(), padding=1, groups=C), TOL_DW)


entry("dwconv3x3 128 19x37 aligned", "dcvc_dwconv3x3")(lambda E: dw_case(E, 128, 19, 37, 4))
entry("dwconv3x3 128 19x37 at offset 2", "dcvc_dwconv3x3")(lambda E: dw_case(E, 128, 19, 37, 2))


# ----------------------------------------------------------------- flow warp
def grids(E, H, W):
    return (E.dev_const(f"gx{W}", lambda: torch.linspace(-1.0, 1.0, W, dtype=torch.float32)),
            E.dev_const(f"gy{H}", lambda: torch.linspace(-1.0, 1.0, H, dtype=torch.float32)))


def warp_fp64(x, flow):
    """grid_sample(bilinear, border, align_corners=True) of x at (col + dx,
    row + dy), in fp64: the sample position clamped to the image, the four
    corners weighted."""
    _, C, H, W = x.shape
    x = x.double()
    px = (torch.arange(W, dtype=torch.float64).view(1, W) + flow[0, 0].double()).clamp(0, W - 1)
    py = (torch.arange(H, dtype=torch.float64).view(H, 1) + flow[0, 1].double()).clamp(0, H - 1)
    x0, y0 = px.floor().long(), py.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    wx, wy = px - x0, py - y0
    g = lambda yy, xx: x[0][:, yy, xx]  # noqa: E731
    out = g(y0, x0) * ((1 - wx) * (1 - wy)) + g(y0, x1) * (wx * (1 - wy)) + g(y1, x0) * ((1 - wx) * wy) \
        + g(y1, x1) * (wx * wy)
    return out.unsqueeze(0)


def warp_case(E, C, H, W, dtype, lead, ylead, ytail, flead, ftail):
    """Dyadic geometry (H - 1, W - 1 powers of two, flows multiples of 1/4
    reaching past every border, integer features below 512): every step of the
    coordinate arithmetic and of the corner sum is exact in fp32, so the
    expected output is the fp64 result itself (rounded once for bf16)."""
    assert (H - 1) & (H - 2) == 0 and (W - 1) & (W - 2) == 0
    x = E.const("x", lambda: torch.randint(-511, 512, (1, C, H, W), generator=seeded("x")).float())
    if dtype == K.BF16:
        x = E.const("xb", lambda: x.bfloat16().float())
    flow = E.const("flow", lambda: torch.randint(-4 * (W + 6), 4 * (W + 6) + 1, (1, 2, H, W),
                                                 generator=seeded("flow")).float() / 4)
    xa = E.x(x, dtype, lead=lead)
    fa = E.x(flow, K.F32, lead=flead, tail=ftail)
    y = E.y("y", C, H, W, dtype, lead=ylead, tail=ytail)
    E.launch(K.flow_warp, xa, fa, grids(E, H, W), y=y)

    def ref():
        r = warp_fp64(x, flow)
        return r.bfloat16().double() if dtype == K.BF16 else r
    E.ref("y", ref, None)


entry("flow_warp fp32 aligned 48 17x33", "dcvc_flow_warp")(lambda E: warp_case(E, 48, 17, 33, K.F32, 8, 8, 8, 8, 6))
entry("flow_warp bf16 aligned 48 17x33", "dcvc_flow_warp")(lambda E: warp_case(E, 48, 17, 33, K.BF16, 8, 8, 8, 8, 6))
# the SpyNet / aux call sites: 3 channels into ch(G1, 3), the flow read from ch(6, 2) of an 8-channel buffer
entry("flow_warp C=3 into ch(48,3), flow from ch(6,2)", "dcvc_flow_warp")(
    lambda E: warp_case(E, 3, 9, 17, K.F32, 0, 48, 5, 6, 0))
entry("flow_warp fp32 at offset 2 48 5x9", "dcvc_flow_warp")(lambda E: warp_case(E, 48, 5, 9, K.F32, 2, 2, 8, 2, 0))


# ---------------------------------------------------------- OffsetDiversity
def bf16_err(got, ref):
    from tests.test_gpu_kernels import bf16_err as f
    return f(got, ref)


def od_case(E, H, W, fdt, odt, lead, planar=False):
    """test_offset_diversity_matches_oracle's restatement (DCVC-DC video_model.py:
    46-61 from the up-sampled offset map onwards) in fp64."""
    from oracle import dc_oracle as O
    rnd = lambda t: t.bfloat16().float()  # noqa: E731
    feat = E.const("feat", lambda: (rnd if fdt == K.BF16 else (lambda t: t))(
        torch.randn(1, 48, H, W, generator=seeded("f"))))
    flow = E.randn("flow", 1, 2, H, W, scale=3.0)
    offs = E.const("offs", lambda: (rnd if odt == K.BF16 else (lambda t: t))(
        torch.randn(1, 96, H // 2, W // 2, generator=seeded("o")) * 0.05))
    fw, fb = E.randn("fw", 48, 6, scale=0.3), E.randn("fb", 48, scale=0.1)
    fa = E.x(feat, fdt, lead=lead, tail=8 if lead % 2 == 0 else 1)
    oa, fl = E.x(offs, odt), E.x(flow, K.F32, lead=6, tail=0)
    y = E.y("y", 48, H, W, fdt, lead=48 if planar else LEAD, tail=0 if planar else LEAD)
    old, K.OD_PLANAR = K.OD_PLANAR, planar
    try:
        E.launch(K.offset_diversity, fa, oa, fl, E.dev_const("fw", lambda: fw), E.dev_const("fb", lambda: fb),
                 grids(E, H, W), y=y)
    finally:
        K.OD_PLANAR = old

    def ref():
        out = O.up2(offs.double())
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        mask = torch.sigmoid(mask)
        offset = 40 * torch.tanh(torch.cat((o1, o2), dim=1)) + flow.double().repeat(1, 32, 1, 1)
        xx = feat.double().view(16, 3, H, W).repeat(2, 1, 1, 1)
        xx = torch.cat([warp_fp64(xx[i:i + 1], offset.view(32, 2, H, W)[i:i + 1]) for i in range(32)]) \
            * mask.view(32, 1, H, W)
        return F.conv2d(xx.view(1, 96, H, W), fw.double().view(48, 6, 1, 1), fb.double(), groups=16)
    if fdt == K.F32:
        E.ref("y", ref, TOL_OD, "abs")
    else:   # a bf16 output: one bf16 rounding of the exact value, TOL_BF16 of test_gpu_kernels.py beyond it
        from tests.test_gpu_kernels import TOL_BF16
        E.ref("y", ref, TOL_BF16, bf16_err)


for _hw in ((6, 2), (10, 130)):
    _s = f"{_hw[0]}x{_hw[1]}"
    entry(f"offset_diversity fp32 pixel-major {_s}", "dcvc_offset_diversity")(
        lambda E, hw=_hw: od_case(E, *hw, K.F32, K.F32, 4))
    entry(f"offset_diversity fp32 planar {_s}", "dcvc_offset_diversity_ws")(
        lambda E, hw=_hw: od_case(E, *hw, K.F32, K.F32, 4, planar=True))
    entry(f"offset_diversity bf16 paired {_s}", "dcvc_offset_diversity")(
        lambda E, hw=_hw: od_case(E, *hw, K.BF16, K.BF16, 8))
    entry(f"offset_diversity bf16 unpaired {_s}", "dcvc_offset_diversity")(
        lambda E, hw=_hw: od_case(E, *hw, K.BF16, K.BF16, 1))
    entry(f"offset_diversity bf16 feature fp32 offsets {_s}", "dcvc_offset_diversity")(
        lambda E, hw=_hw: od_case(E, *hw, K.BF16, K.F32, 8))


# --------------------------------------------------------------- resampling
@entry("resize2x up x2.0 into ch(6,2) 7x11", "dcvc_resize2x")
def _up(E, H=7, W=11):
    x = E.randn("x", 1, 2, H, W)
    xa, y = E.x(x, lead=2, tail=0), E.y("y", 2, 2 * H, 2 * W, lead=6, tail=0)
    E.launch(K.resize2x, xa, True, 2.0, y=y)
    E.ref("y", lambda: F.interpolate(x.double(), (2 * H, 2 * W), mode="bilinear", align_corners=False) * 2.0,
          TOL_RESAMPLE, "abs")


def down2_ref(x, oh, ow):
    """bilineardownsacling = F.interpolate(bilinear, align_corners=False) as ATen
    defines it for an fp32 map: the source position scale * (dst + 0.5) - 0.5,
    scale = in / out, is computed in the map's own type, fp32; that position is
    part of the operation (for an odd size it is no dyadic number), so the
    restatement takes it as defined and blends the four neighbours in fp64.
    With the positions in fp64 as well, the odd-size case differs from the
    kernel AND from the fp32 reference op by up to 1.8e-6 (the position's fp32
    rounding times the map's gradient), above this family's 1e-6."""
    def axis(n_in, n_out):
        sc = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
        s = (sc * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
        i0 = s.floor().long()
        return i0, (i0 + 1).clamp(max=n_in - 1), (s - i0.float()).double()
    (h0, h1, hl), (w0, w1, wl) = axis(x.shape[2], oh), axis(x.shape[3], ow)
    xd = x.double()
    hl, wl = hl.view(1, 1, -1, 1), wl.view(1, 1, 1, -1)
    g = lambda hh, ww: xd[:, :, hh][:, :, :, ww]  # noqa: E731
    return (g(h0, w0) * (1 - wl) + g(h0, w1) * wl) * (1 - hl) + (g(h1, w0) * (1 - wl) + g(h1, w1) * wl) * hl


@entry("resize2x down x0.5 from 15x23", "dcvc_resize2x")
def _down(E, H=15, W=23, C=5):
    x = E.randn("x", 1, C, H, W)
    xa, y = E.x(x), E.y("y", C, H // 2, W // 2)
    E.launch(K.resize2x, xa, False, 0.5, y=y)
    E.ref("y", lambda: down2_ref(x, H // 2, W // 2) * 0.5, TOL_RESAMPLE, "abs")


def pool_case(E, is_max, H=15, W=23, C=5):
    x = E.randn("x", 1, C, H, W)
    xa, y = E.x(x), E.y("y", C, H // 2, W // 2)
    E.launch(K.pool2x2, xa, is_max, y=y)
    if is_max:
        E.ref("y", lambda: F.max_pool2d(x.double(), 2, 2), None)
    else:
        E.ref("y", lambda: F.avg_pool2d(x.double(), 2, 2), TOL_RESAMPLE, "abs")


entry("pool2x2 max from 15x23", "dcvc_pool2x2")(lambda E: pool_case(E, True))
entry("pool2x2 avg from 15x23", "dcvc_pool2x2")(lambda E: pool_case(E, False))


# -------------------------------------------------- elementwise and copies
def ew_case(E, op, lead, dt=K.F32, C=48, H=9, W=13):
    """test_copy_and_pad_views: exact copies (with dtype conversion), replicate
    padding; dcvc_add: one fp32 add, exact against fp64 rounded once."""
    tdt = torch.float32 if dt == K.F32 else torch.bfloat16
    x = E.const("x", lambda: torch.randn(1, C, H, W, generator=seeded("x")).to(tdt).float())
    xa = E.x(x, dt, lead=lead)
    if op == "copy":
        y = E.y("y", C, H, W, dt, lead=lead)
        E.launch(K.copy, xa, y)
        E.ref("y", lambda: x.double(), None)
    elif op == "copy_cvt":      # fp32 -> bf16
        y = E.y("y", C, H, W, K.BF16, lead=lead)
        E.launch(K.copy, xa, y)
        E.ref("y", lambda: x.bfloat16().double(), None)
    elif op == "pad":
        y = E.y("y", C, H + 5, W + 3, dt, lead=lead)
        E.launch(K.pad_replicate, xa, y)
        E.ref("y", lambda: F.pad(x.double(), (0, 3, 0, 5), mode="replicate"), None)
    elif op == "add":
        b = E.const("b", lambda: torch.randn(1, C, H, W, generator=seeded("b")).to(tdt).float())
        ba, y = E.x(b, dt, lead=lead), E.y("y", C, H, W, dt, lead=lead)
        E.launch(K.add, xa, ba, y=y)
        E.ref("y", lambda: (x.double() + b.double()).to(tdt).double(), None)


for _lead in (8, 2):
    _s = "aligned" if _lead == 8 else "at offset 2"
    entry(f"copy fp32 {_s}", "dcvc_copy")(lambda E, l=_lead: ew_case(E, "copy", l))
    entry(f"copy fp32->bf16 {_s}", "dcvc_copy")(lambda E, l=_lead: ew_case(E, "copy_cvt", l))
    entry(f"pad_replicate fp32 {_s}", "dcvc_pad_replicate")(lambda E, l=_lead: ew_case(E, "pad", l))
    entry(f"add fp32 {_s}", "dcvc_add")(lambda E, l=_lead: ew_case(E, "add", l))
entry("add bf16 aligned", "dcvc_add")(lambda E: ew_case(E, "add", 8, K.BF16))


def fill_case(E, lead, dt):
    y = E.y("y", 5, 9, 13, dt, lead=lead)
    E.launch(K.fill, y, 1.5)
    E.ref("y", lambda: torch.full((1, 5, 9, 13), 1.5, dtype=torch.float64), None)


entry("fill fp32 window", "dcvc_fill")(lambda E: fill_case(E, 3, K.F32))
entry("fill bf16 window", "dcvc_fill")(lambda E: fill_case(E, 8, K.BF16))


@entry("channel_div 5 9x13", "dcvc_channel_div")
def _cdiv(E, C=5, H=9, W=13):
    """test_channel_div_is_a_true_division: the correctly rounded fp32 quotient."""
    x = E.randn("x", 1, C, H, W, scale=7.0)
    q = E.const("q", lambda: torch.rand(C, generator=seeded("q")) * 2.5 + 0.5)
    xa, y = E.x(x, lead=1, tail=3), E.y("y", C, H, W, lead=3, tail=3)
    E.launch(K.channel_div, xa, E.dev_const("q", lambda: q), y)
    E.ref("y", lambda: (x / q.view(1, -1, 1, 1)).double(), None)


def se_case(E, C, lead, H=45, W=77):
    """test_se_layer_matches_torch (fp32: scale to 1e-5 absolute, apply to 1e-5 rel_err)."""
    Rr = max(1, C // 16)
    x, a = E.randn("x", 1, C, H, W), E.randn("a", 1, C, H, W)
    w1, w2 = E.randn("w1", Rr, C, scale=0.3), E.randn("w2", C, Rr, scale=0.3)
    xa, aa = E.x(x, lead=lead), E.x(a)
    work = E.scratch(256 * C, torch.float32)
    s = E.yraw("scale", C, torch.float32)
    y = E.y("y", C, H, W)
    E.launch(K.se_scale, xa, E.dev_const("w1", lambda: w1), E.dev_const("w2", lambda: w2), work, s)
    E.launch(K.se_apply, aa, xa, s, y=y)
    ref_s = lambda: torch.sigmoid(w2.double() @ torch.relu(w1.double() @ x.double().mean((-1, -2))[0]))  # noqa: E731
    E.ref("scale", ref_s, TOL_SE, "abs")
    E.ref("y", lambda: a.double() + x.double() * ref_s()[None, :, None, None], TOL_SE)


entry("se_scale + se_apply 64 45x77 aligned", "dcvc_se_scale", "dcvc_se_apply")(lambda E: se_case(E, 64, 8))
entry("se_scale + se_apply 36 45x77 at offset 3", "dcvc_se_scale", "dcvc_se_apply")(lambda E: se_case(E, 36, 3))


# ---------------------------------------------------------------- frame I/O
FRAME = (38, 54, 48, 64)      # h, w, H, W of test_harness.py / test_crossfmt.py SHAPES[1]


def u8(E, key, *shape):
    return E.const(key, lambda: torch.randint(0, 256, shape, generator=seeded(key)).to(torch.uint8))


def frame_case(E, zero_pad):
    """test_frame_to_nhwc_padding."""
    h, w, H, W = FRAME
    src = u8(E, "src", 3, h, w)
    y = E.y("y", 3, H, W, lead=0, tail=0)
    E.launch(K.frame_to_nhwc, E.raw(src), h, w, y, zero_pad=zero_pad)
    r = src.float().unsqueeze(0) / 255.0
    E.ref("y", lambda: F.pad(r, (0, W - w, 0, H - h), mode="constant" if zero_pad else "replicate").double(), None)


entry("frame_to_nhwc replicate", "dcvc_frame_to_nhwc")(lambda E: frame_case(E, False))
entry("frame_to_nhwc zero pad", "dcvc_frame_to_nhwc_zero_pad")(lambda E: frame_case(E, True))


def hwc(a):
    """(H, W, C) numpy -> (1, C, H, W) fp64 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).unsqueeze(0).double()


@entry("yuv420_to_nhwc", "dcvc_yuv420_to_nhwc")
def _yuv_in(E):
    from oracle import harness_oracle as HO
    h, w, H, W = FRAME
    yp, uv = u8(E, "y", h, w), u8(E, "uv", 2, h // 2, w // 2)
    out = E.y("y", 3, H, W, lead=0, tail=0)
    E.launch(K.yuv420_to_nhwc, E.raw(yp), E.raw(uv), h, w, out)
    E.ref("y", lambda: hwc(HO.yuv_u8_to_input(yp.numpy(), uv.numpy(), H, W)), None)


@entry("yuv420_to_rgb_nhwc", "dcvc_yuv420_to_rgb_nhwc")
def _yuv_rgb(E):
    from tests import crossfmt_ref as C
    h, w, H, W = FRAME
    yp, uv = u8(E, "y", h, w), u8(E, "uv", 2, h // 2, w // 2)
    out = E.y("y", 3, H, W, lead=0, tail=0)
    planes = E.yraw("planes", 3 * h * w, torch.float32)
    E.launch(K.yuv420_to_rgb_nhwc, E.raw(yp), E.raw(uv), h, w, out, planes)
    ref = lambda: C.ingest_yuv_source_rgb_codec(yp.numpy(), uv.numpy(), H, W)  # noqa: E731
    E.ref("y", lambda: hwc(ref()[0]), None)
    E.ref("planes", lambda: torch.from_numpy(ref()[1]).reshape(-1), None)


@entry("rgb_to_yuv420_planes + yuv420f_to_nhwc", "dcvc_rgb_to_yuv420_planes", "dcvc_yuv420f_to_nhwc")
def _rgb_yuv(E):
    from tests import crossfmt_ref as C
    h, w, H, W = FRAME
    rgb = u8(E, "rgb", 3, h, w)
    yf, uvf = E.yraw("yf", h * w, torch.float32), E.yraw("uvf", 2 * (h // 2) * (w // 2), torch.float32)
    out = E.y("y", 3, H, W, lead=0, tail=0)
    E.launch(K.rgb_to_yuv420_planes, E.raw(rgb), h, w, yf, uvf)
    E.launch(K.yuv420f_to_nhwc, yf, uvf, h, w, out)
    ref = lambda: C.ingest_rgb_source_yuv_codec(rgb.numpy(), H, W)  # noqa: E731
    E.ref("y", lambda: hwc(ref()[0]), None)
    E.ref("yf", lambda: torch.from_numpy(ref()[1]).reshape(-1), None)
    E.ref("uvf", lambda: torch.from_numpy(ref()[2]).reshape(-1), None)


def recon(E):
    h, w, H, W = FRAME
    return E.const("xh", lambda: (torch.rand(1, 3, H, W, generator=seeded("xh")) * 1.2 - 0.1))


def recon_u8_case(E, yuv420, cross):
    """test_recon_writers_match_reference_formulas / test_recon_to_u8_cross_matches_restatement."""
    from oracle import harness_oracle as HO
    from tests import crossfmt_ref as C
    h, w, H, W = FRAME
    xh = recon(E)
    n = h * w + 2 * (h // 2) * (w // 2) if (not cross and yuv420) or (cross and not yuv420) else 3 * h * w
    out = E.yraw("u8", n, torch.uint8)
    xa = E.x(xh, lead=0, tail=0)
    if cross:
        E.launch(K.recon_to_u8_cross, xa, h, w, yuv420, out)      # yuv420 here: x_hat holds YCbCr (to_rgb)
    else:
        E.launch(K.recon_to_u8, xa, h, w, yuv420, out)
    crop = np.ascontiguousarray(xh[0, :, :h, :w].numpy())

    def ref():
        if cross:
            b = C.png_bytes_from_444(crop).tobytes() if yuv420 else C.yuv_bytes_from_rgb(crop)
        elif yuv420:
            b = HO.yuv_writer_bytes(*HO.ycbcr444_to_420(crop))
        else:
            b = HO.png_writer_u8(crop).tobytes()
        return torch.frombuffer(bytearray(b), dtype=torch.uint8)
    E.ref("u8", ref, None)


entry("recon_to_u8 rgb", "dcvc_recon_to_u8")(lambda E: recon_u8_case(E, False, False))
entry("recon_to_u8 yuv420", "dcvc_recon_to_u8")(lambda E: recon_u8_case(E, True, False))
entry("recon_to_u8_cross to rgb", "dcvc_recon_to_u8_cross")(lambda E: recon_u8_case(E, True, True))
entry("recon_to_u8_cross to yuv420", "dcvc_recon_to_u8_cross")(lambda E: recon_u8_case(E, False, True))


# ------------------------------------------------------------------ metrics
def sse_case(E, yuv, f32):
    """test_frame_sse_and_inplace_clamp / test_frame_sse_f32_and_inplace_clamp:
    the three sums to rtol 1e-12, x_hat clamped in place over the whole buffer."""
    from oracle import harness_oracle as HO
    h, w, H, W = FRAME
    xh = E.const("xh", lambda: torch.rand(1, 3, H, W, generator=seeded("xh")) * 1.4 - 0.2)
    xa = E.inout("x_hat", xh, lead=0, tail=0)
    ws = E.scratch(int(K.lib().dcvc_frame_sse_workspace()) // 8, torch.float64) if not E.dry else None
    out = E.yraw("sse", 3, torch.float64)
    crop = np.ascontiguousarray(xh.clamp(0, 1)[0, :, :h, :w].numpy())
    if yuv:
        yp, uv = u8(E, "y", h, w), u8(E, "uv", 2, h // 2, w // 2)
        if f32:
            yp, uv = E.const("yf", lambda: yp.float() / 255), E.const("uvf", lambda: uv.float() / 255)
            E.launch(K.frame_sse_f32, xa, E.raw(yp), h, w, ws, out, uv_f32=E.raw(uv))
        else:
            E.launch(K.frame_sse, xa, E.raw(yp), h, w, ws, out, uv_u8=E.raw(uv))

        def ref():
            y_rec, uv_rec = HO.ycbcr444_to_420(crop)
            sy, suv = (yp.numpy(), uv.numpy()) if f32 else (yp.numpy().astype(np.float32) / 255,
                                                            uv.numpy().astype(np.float32) / 255)
            e = [y_rec[0].astype(np.float64) - sy, uv_rec[0].astype(np.float64) - suv[0],
                 uv_rec[1].astype(np.float64) - suv[1]]
            return torch.tensor([np.sum(np.square(v)) for v in e], dtype=torch.float64)
    else:
        src = u8(E, "src", 3, h, w)
        if f32:
            src = E.const("srcf", lambda: src.float() / 255)
            E.launch(K.frame_sse_f32, xa, E.raw(src), h, w, ws, out)
        else:
            E.launch(K.frame_sse, xa, E.raw(src), h, w, ws, out)

        def ref():
            s = src.numpy() if f32 else src.numpy().astype(np.float32) / np.float32(255)
            d = crop - s
            return torch.tensor([np.sum((d[c] * d[c]).astype(np.float64)) for c in range(3)], dtype=torch.float64)
    E.ref("sse", ref, TOL_SSE, "rtol")
    E.ref("x_hat", lambda: xh.clamp(0, 1).double(), None)


entry("frame_sse rgb", "dcvc_frame_sse")(lambda E: sse_case(E, False, False))
entry("frame_sse yuv420", "dcvc_frame_sse")(lambda E: sse_case(E, True, False))
entry("frame_sse_f32 rgb", "dcvc_frame_sse_f32")(lambda E: sse_case(E, False, True))
entry("frame_sse_f32 yuv420", "dcvc_frame_sse_f32")(lambda E: sse_case(E, True, True))


def planes_case(E, yuv, f32):
    """calc_msssim's fp64 inputs: the source planes (uint8 / 255 in fp32, or
    the fp32 planes) and the clamped recon's planes, exact."""
    from oracle import harness_oracle as HO
    h, w, H, W = FRAME
    xh = recon(E)
    xa = E.x(xh, lead=0, tail=0)
    n = h * w + 2 * (h // 2) * (w // 2) if yuv else 3 * h * w
    src, rec = E.yraw("src", n, torch.float64), E.yraw("rec", n, torch.float64)
    crop = np.ascontiguousarray(xh.clamp(0, 1)[0, :, :h, :w].numpy())
    if yuv:
        yp, uv = u8(E, "y", h, w), u8(E, "uv", 2, h // 2, w // 2)
        yf, uvf = E.const("yf", lambda: yp.float() / 255), E.const("uvf", lambda: uv.float() / 255)
        if f32:
            E.launch(K.yuv_planes_f64_f32, xa, E.raw(yf), E.raw(uvf), h, w, src, rec)
        else:
            E.launch(K.yuv_planes_f64, xa, E.raw(yp), E.raw(uv), h, w, src, rec)
        E.ref("src", lambda: torch.cat([yf.reshape(-1), uvf.reshape(-1)]).double(), None)

        def rref():
            y_rec, uv_rec = HO.ycbcr444_to_420(crop)
            return torch.from_numpy(np.concatenate([y_rec.reshape(-1), uv_rec.reshape(-1)])).double()
        E.ref("rec", rref, None)
    else:
        s8 = u8(E, "src", 3, h, w)
        sf = E.const("srcf", lambda: s8.float() / 255)
        if f32:
            E.launch(K.rgb_planes_f64_f32, xa, E.raw(sf), h, w, src, rec)
        else:
            E.launch(K.rgb_planes_f64, xa, E.raw(s8), h, w, src, rec)
        E.ref("src", lambda: sf.reshape(-1).double(), None)
        E.ref("rec", lambda: torch.from_numpy(crop.reshape(-1)).double(), None)


entry("yuv_planes_f64", "dcvc_yuv_planes_f64")(lambda E: planes_case(E, True, False))
entry("yuv_planes_f64_f32", "dcvc_yuv_planes_f64_f32")(lambda E: planes_case(E, True, True))
entry("rgb_planes_f64", "dcvc_rgb_planes_f64")(lambda E: planes_case(E, False, False))
entry("rgb_planes_f64_f32", "dcvc_rgb_planes_f64_f32")(lambda E: planes_case(E, False, True))


@entry("ssim_level 37x53", "dcvc_ssim_level")
def _ssim(E, h=37, w=53):
    """calc_ssim's two means (test_gpu_msssim_matches_reference_fixtures: 1e-10)."""
    from oracle import harness_oracle as HO
    a = E.const("a", lambda: torch.rand(h, w, generator=seeded("a"), dtype=torch.float64))
    b = E.const("b", lambda: (a + 0.05 * torch.randn(h, w, generator=seeded("b"), dtype=torch.float64)).clamp(0, 1))
    win = E.dev_const("win", lambda: torch.from_numpy(HO.fspecial_gauss(11, 1.5)))
    ws = E.scratch(int(K.lib().dcvc_ssim_workspace()) // 8, torch.float64) if not E.dry else None
    out = E.yraw("out2", 2, torch.float64)
    E.launch(K.ssim_level, E.raw(a), E.raw(b), h, w, win, ws, out)
    E.ref("out2", lambda: torch.tensor(HO.calc_ssim(a.numpy(), b.numpy()), dtype=torch.float64), TOL_SSIM, "abs")


@entry("down2_f64 from 11x13", "dcvc_down2_f64")
def _down2(E, h=11, w=13):
    """test_down2_reflect_matches_scipy's restatement (atol 1e-15)."""
    from oracle import harness_oracle as HO
    a = E.const("a", lambda: torch.rand(h, w, generator=seeded("a"), dtype=torch.float64))
    out = E.yraw("out", ((h + 1) // 2) * ((w + 1) // 2), torch.float64)
    E.launch(K.down2_f64, E.raw(a), h, w, out)
    E.ref("out", lambda: torch.from_numpy(HO.down2_reflect(a.numpy())).reshape(-1), 1e-15, "abs")


@entry("avgpool2_f64 from 11x13", "dcvc_avgpool2_f64")
def _avg2(E, h=11, w=13):
    """test_avgpool2_padding_semantics: avg_pool2d(kernel 2, padding size % 2, count_include_pad), exact in fp64."""
    a = E.const("a", lambda: torch.randint(0, 1 << 20, (h, w), generator=seeded("a")).double() / (1 << 20))
    oh, ow = (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1
    out = E.yraw("out", oh * ow, torch.float64)
    E.launch(K.avgpool2_f64, E.raw(a), h, w, out)
    E.ref("out", lambda: F.avg_pool2d(a[None, None], kernel_size=2, padding=[h % 2, w % 2]).reshape(-1), None)


@entry("sum_f32 1025", "dcvc_sum_f32")
def _sum(E, n=1025):
    """test_sum_f32's bound: (ceil(n / 1024) + 10) 2^-24 sum |x|."""
    x = E.const("x", lambda: torch.randn(n, generator=seeded("x"))
                * torch.exp(torch.rand(n, generator=seeded("e")) * 6 - 3))
    out = E.yraw("out", 1, torch.float32)
    E.launch(K.sum_f32, E.raw(x), out)
    bound = (-(-n // 1024) + 10) * 2.0 ** -24 * x.double().abs().sum().item()
    E.ref("out", lambda: x.double().sum().reshape(1), bound, "abs")


def bits_bad(name):
    """Elements outside check_bits' per-element bound of test_gpu_entropy_kernels.py (must be 0)."""
    def f(got, p):
        from tests.test_gpu_entropy_kernels import k_gpu
        g, pp = got.numpy().astype(np.float64).reshape(-1), p.numpy().reshape(-1)
        return float((np.abs(g - R.probs_to_bits(pp)) > R.bits_bound(pp, k_gpu(name))).sum())
    return f


@entry("factorized_bits 5 9x13", "dcvc_factorized_bits")
def _fact(E, shape=(5, 9, 13)):
    C, H, W = shape
    case = E.const("case", lambda: R.factorized_case(*shape))
    z = E.x(torch.from_numpy(case["z"])[None], lead=3, tail=1)
    bits = E.yraw("bits", C * H * W, torch.float32)
    E.launch(K.factorized_bits, z, E.dev_const("table", lambda: torch.from_numpy(case["table"])), bits)
    E.ref("bits", lambda: torch.from_numpy(R.factorized_prob(case["z"], case["table"]).transpose(1, 2, 0).reshape(-1)),
          1.0, bits_bad("factorized"))


# ------------------------------------------------------------------ entropy
def chw(a):
    return torch.from_numpy(np.ascontiguousarray(a))[None]


def idx_bad(got, v):
    """Indexes that differ from clamp(trunc(v)) away from a tie (check_indexes
    of test_gpu_entropy_kernels.py: none; within IDX_TIE_EPS of an integer +-1)."""
    v = v.numpy()
    ref, near = R.index_of(v), R.near_integer(v, R.IDX_TIE_EPS)
    d = got.numpy().astype(np.int64) - ref
    return float((d[~near] != 0).sum() + (np.abs(d[near]) > 1).sum())


QT = (12, 5, 7)      # R.QT_SHAPES[1]


def qt_case(E, mode):
    """The four quadtree steps in order on the production layout (params at
    ch(C, 3C) and y_hat_so_far at ch(0, C) of one buffer): symbols, y_hat and
    y_hat_so_far bit for bit, indexes as check_indexes, bits as check_bits."""
    C, H, W = QT
    est = mode.startswith("estimate")
    case = E.const("case", lambda: R.quadtree_case(*QT, est=est))
    steps = E.const("steps", lambda: R.quadtree_run(case["params"], case["sms"], y=case["y"])[0])
    lm, ls = R.LAPLACE_TABLE
    n = C // 4 * H * W
    sp = E.inout("sp", chw(np.concatenate([np.zeros((C, H, W), np.float32), case["params"]])), lead=4, tail=4)
    yhs, params = sp.ch(0, C), sp.ch(C, 3 * C)
    sms = [E.x(chw(s), lead=1, tail=3) for s in case["sms"]]
    ya = E.x(chw(case["y"]), lead=1, tail=1) if mode != "decode" and mode != "indexes" else None
    yhat = E.y("yhat", C, H, W, lead=3, tail=2) if mode != "indexes" else None
    exp_yhs, exp_yhat = np.zeros((C, H, W), np.float32), np.zeros((C, H, W), np.float32)
    for k in range(4):
        sm = None if k == 0 else sms[k - 1]
        st = steps[k]
        R.scatter(exp_yhs, st["ch"], st["yhs"])
        R.scatter(exp_yhat, st["ch"], st["yhat"])
        sym_ref = torch.from_numpy(st["sym"].reshape(-1).astype(np.int16))
        idx_v = torch.from_numpy(R.index_float64(st["scale"].reshape(-1), lm, ls))
        if mode == "encode":
            sym, idx = E.yraw(f"sym{k}", n, torch.int16), E.yraw(f"idx{k}", n, torch.int16)
            E.launch(K.qt_encode_step, ya, params, sm, k, yhs, yhat, sym, idx, lm, ls)
            E.ref(f"sym{k}", lambda s=sym_ref: s, None)
            E.ref(f"idx{k}", lambda v=idx_v: v, 1.0, idx_bad)
        elif mode == "indexes":
            idx = E.yraw(f"idx{k}", n, torch.int16)
            E.launch(K.qt_indexes_step, params, sm, k, idx, lm, ls)
            E.ref(f"idx{k}", lambda v=idx_v: v, 1.0, idx_bad)
        elif mode == "decode":
            E.launch(K.qt_decode_step, params, sm, k, E.raw(sym_ref), yhs, yhat)
        else:
            gaussian = mode.endswith("normal")
            bits = E.yraw(f"bits{k}", n, torch.float32)
            E.launch(K.qt_estimate_step, ya, params, sm, k, yhs, yhat, bits, gaussian)
            prob = R.normal_prob if gaussian else R.laplace_prob
            E.ref(f"bits{k}", lambda s=st, f=prob: torch.from_numpy(f(s["sym_f"], s["scale"], 1e-5).reshape(-1)),
                  1.0, bits_bad("normal_dc" if gaussian else "laplace"))
    if mode == "indexes":
        E.ref("sp", lambda: chw(np.concatenate([np.zeros((C, H, W), np.float32), case["params"]])).double(), None)
        return
    if mode == "decode":     # the decoder sees the clamped symbols
        d = R.quadtree_run(case["params"], case["sms"], syms=[s["sym"] for s in steps])[0]
        exp_yhs, exp_yhat = np.zeros((C, H, W), np.float32), np.zeros((C, H, W), np.float32)
        for st in d:
            R.scatter(exp_yhs, st["ch"], st["yhs"])
            R.scatter(exp_yhat, st["ch"], st["yhat"])
    E.ref("yhat", lambda: chw(exp_yhat).double(), None)
    E.ref("sp", lambda: chw(np.concatenate([exp_yhs, case["params"]])).double(), None)


entry("quadtree encode steps k=0..3", "dcvc_quadtree_encode_step")(lambda E: qt_case(E, "encode"))
entry("quadtree indexes steps k=0..3", "dcvc_quadtree_indexes_step")(lambda E: qt_case(E, "indexes"))
entry("quadtree decode steps k=0..3", "dcvc_quadtree_decode_step")(lambda E: qt_case(E, "decode"))
entry("quadtree estimate steps k=0..3 laplace", "dcvc_quadtree_estimate_step")(lambda E: qt_case(E, "estimate laplace"))
entry("quadtree estimate steps k=0..3 normal", "dcvc_quadtree_estimate_step")(lambda E: qt_case(E, "estimate normal"))

DP = (6, 4, 6)       # R.DP_SHAPES[1]


def dp_case(E, mode):
    """The two dual-prior steps in order, with post_scale (the issue's k = 0..3
    are the quadtree's: the checkerboard has two steps)."""
    C, H, W = DP
    est = mode.startswith("estimate")
    case = E.const("case", lambda: R.dual_case(*DP, est=est))
    steps = E.const("steps", lambda: R.dual_run(case["buf"], case["sm"], y=case["y"], post=case["post"])[0])
    lm, ls = R.NORMAL_TABLE
    n = C // 2 * H * W
    buf = E.inout("buf", chw(case["buf"]), lead=1, tail=1)
    sm_a = E.x(chw(case["sm"]), lead=1, tail=3)
    ya = E.x(chw(case["y"]), lead=1, tail=1) if mode not in ("decode", "indexes") else None
    yhat = E.y("yhat", C, H, W, lead=3, tail=2) if mode != "indexes" else None
    post = E.raw(torch.from_numpy(case["post"]))
    exp_yhat = np.zeros((C, H, W), np.float32)
    for k in range(2):
        sm = None if k == 0 else sm_a
        st = steps[k]
        R.scatter(exp_yhat, st["ch"], st["yhat"])
        sym_ref = torch.from_numpy(st["sym_f"].reshape(-1).astype(np.int32))
        idx_v = torch.from_numpy(R.index_float64(st["scale"].reshape(-1), lm, ls))
        if mode == "encode":
            sym, idx = E.yraw(f"sym{k}", n, torch.int32), E.yraw(f"idx{k}", n, torch.int16)
            E.launch(K.dp_encode_step, ya, buf, sm, k, yhat, post, sym, idx, lm, ls)
            E.ref(f"sym{k}", lambda s=sym_ref: s, None)
            E.ref(f"idx{k}", lambda v=idx_v: v, 1.0, idx_bad)
        elif mode == "indexes":
            idx = E.yraw(f"idx{k}", n, torch.int16)
            E.launch(K.dp_indexes_step, buf, sm, k, idx, lm, ls)
            E.ref(f"idx{k}", lambda v=idx_v: v, 1.0, idx_bad)
        elif mode == "decode":
            E.launch(K.dp_decode_step, buf, sm, k, E.raw(sym_ref), yhat, post)
        else:
            gaussian = mode.endswith("normal")
            smin = 0.11 if gaussian else 1e-5
            bits = E.yraw(f"bits{k}", n, torch.float32)
            E.launch(K.dp_estimate_step, ya, buf, sm, k, yhat, post, bits, gaussian, smin)
            prob = R.normal_prob if gaussian else R.laplace_prob
            E.ref(f"bits{k}", lambda s=st, f=prob, m=smin: torch.from_numpy(f(s["sym_f"], s["scale"], m).reshape(-1)),
                  1.0, bits_bad("normal_hem" if gaussian else "laplace"))
    if mode == "indexes":
        return
    E.ref("yhat", lambda: chw(exp_yhat).double(), None)
    E.ref("buf", lambda: chw(steps[0]["buf"]).double(), None)


entry("dual prior encode steps k=0..1", "dcvc_dual_prior_encode_step")(lambda E: dp_case(E, "encode"))
entry("dual prior indexes steps k=0..1", "dcvc_dual_prior_indexes_step")(lambda E: dp_case(E, "indexes"))
entry("dual prior decode steps k=0..1", "dcvc_dual_prior_decode_step")(lambda E: dp_case(E, "decode"))
entry("dual prior estimate steps k=0..1 normal", "dcvc_dual_prior_estimate_step")(
    lambda E: dp_case(E, "estimate normal"))
entry("dual prior estimate steps k=0..1 laplace", "dcvc_dual_prior_estimate_step")(
    lambda E: dp_case(E, "estimate laplace"))

TSHAPE = (5, 9, 13)      # test_gpu_entropy_kernels.py: three blocks, the last one partial


def sym_case(E, wide, back):
    """The symbol transposes: NHWC float <-> NCHW integers, exact."""
    C, H, W = TSHAPE
    n = C * H * W
    limit = 2 ** 24 if wide else 29000
    v = E.const("v", lambda: torch.randint(-limit, limit + 1, (1, C, H, W), generator=seeded("v")))
    it = torch.int32 if wide else torch.int16
    if back:
        y = E.y("y", C, H, W, lead=3, tail=3)
        E.launch(K.from_symbols_i32 if wide else K.from_symbols, E.raw(v.reshape(-1).to(it)), y)
        E.ref("y", lambda: v.double(), None)
    else:
        sym = E.yraw("sym", n, it)
        E.launch(K.to_symbols_i32 if wide else K.to_symbols, E.x(v.float(), lead=3, tail=3), sym)
        E.ref("sym", lambda: v.reshape(-1).to(it), None)


entry("nhwc_to_symbols", "dcvc_nhwc_to_symbols")(lambda E: sym_case(E, False, False))
entry("symbols_to_nhwc", "dcvc_symbols_to_nhwc")(lambda E: sym_case(E, False, True))
entry("nhwc_to_symbols_i32", "dcvc_nhwc_to_symbols_i32")(lambda E: sym_case(E, True, False))
entry("symbols_i32_to_nhwc", "dcvc_symbols_i32_to_nhwc")(lambda E: sym_case(E, True, True))


# ------------------------------------------------------------------- digest
def digest_case(E, dt, lead, C=48, H=9, W=13):
    """ref_digest of test_gpu_digest.py on the view's bit patterns, folded into zeros."""
    from tests.test_gpu_digest import ref_digest, M64
    tdt = torch.float32 if dt == K.F32 else torch.bfloat16
    x = E.const("x", lambda: (torch.randn(1, C, H, W, generator=seeded("x")) * 3).to(tdt).float())
    xa = E.x(x, dt, lead=lead)
    out = E.yraw("out", 2, torch.int64, init=torch.zeros(2, dtype=torch.int64))
    ws = E.scratch(int(K.lib().dcvc_digest_workspace()) // 8, torch.int64) if not E.dry else None
    E.launch(K.digest, xa, 5, out, ws)

    def ref():
        t = x[0].permute(1, 2, 0).contiguous().to(tdt)
        bits = (t.view(torch.int32).numpy().view(np.uint32) if dt == K.F32
                else t.view(torch.int16).numpy().view(np.uint16))
        s, xo = ref_digest(bits, 5)
        return torch.from_numpy(np.array([s & M64, xo & M64], dtype=np.uint64).view(np.int64))
    E.ref("out", ref, None)


entry("digest fp32 aligned", "dcvc_digest")(lambda E: digest_case(E, K.F32, 8))
entry("digest fp32 at offset 2", "dcvc_digest")(lambda E: digest_case(E, K.F32, 2))
entry("digest bf16 aligned", "dcvc_digest")(lambda E: digest_case(E, K.BF16, 8))


# ---------------------------------------------------------------- the tests
# Launchers with a tensor argument that the table leaves out, and why.
EXCLUDED = {}


def tensor_launchers():
    """The symbols of hip.HIP_SYMBOLS with a CTensor or args-struct parameter."""
    out = []
    for name, _, args in K.HIP_SYMBOLS:
        for a in args:
            if a is K.CTensor or (isinstance(a, type) and issubclass(a, ctypes._Pointer)
                                  and issubclass(a._type_, ctypes.Structure)):
                out.append(name)
                break
    return out


def test_every_launcher_has_a_hygiene_case():
    covered = {s for _, syms, _, _ in TABLE.values() for s in syms}
    names = tensor_launchers()
    assert "dcvc_conv2d" in names and "dcvc_copy" in names and "dcvc_conv_ffn" in names
    assert "dcvc_conv_pack_weights" not in names and "dcvc_sum_f32" not in names
    missing = [n for n in names if n not in covered and n not in EXCLUDED]
    assert not missing, f"launchers without a hygiene table entry or an EXCLUDED reason: {missing}"
    both = [n for n in EXCLUDED if n in covered]
    assert not both, both
    known = {n for n, _, _ in K.HIP_SYMBOLS}
    assert covered <= known and set(EXCLUDED) <= known, sorted((covered | set(EXCLUDED)) - known)
    assert all(isinstance(r, str) and r for r in EXCLUDED.values())
    # launchers without a tensor argument (pack functions, workspace queries, option and debug calls) need no case
    assert not {"dcvc_ffn_pack_weights", "dcvc_digest_workspace", "dcvc_debug_poison_lds",
                "dcvc_set_option"} & set(names)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_entry_builds_on_the_cpu(name):
    """Every entry builds its call and its references without a device (the
    launches skipped): each reference has the shape of the output it is for."""
    fn, _, _, _ = TABLE[name]
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
    fn, _, guard, deterministic = TABLE[name]
    try:
        routes = HY.run_entry(fn, name, guard=guard, deterministic=deterministic)
    finally:
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:     # a GPU error poisons the process: launch nothing more
            pytest.exit(f"GPU error, stopping: {e}", returncode=3)
    print(f"hygiene-route {name!r}: {sorted(set(routes))}")

"""The judge of tests/test_gpu_conv_conformance.py, checked without a GPU.

conv_cases.reference() decides whether a kernel is right, so it is itself
held to a straight-line torch composition (F.conv2d, F.leaky_relu,
F.pixel_shuffle in fp64) on three small cases; the generated data must tell
the errors a kernel is likely to make apart from rounding (each moves the
result by more than 100 times the case's bound); and every case of the table
must have a conformance parametrisation and a golden route.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as CC
from tests.conv_cases import C, CASES

BY_NAME = {c["name"]: c for c in CASES}
# the bounds of tests/test_gpu_conv_conformance.py (restated: that module's
# imports are GPU test modules)
BOUND = {"f16x3": 4e-6, "f32": 2e-5, "bf16": 1e-4}


def formula(c, t, in_lrelu=None, drop_res2=False, scale_unshuffled=False, no_clamp=False, half_away=False):
    """y of the call as a straight-line torch composition in fp64, (Hy, Wy, cy);
    the keywords put one deliberate error each into it."""
    g = CC.geometry(c)
    x = t["x"][:, :, g["xoff"]:g["xoff"] + g["cx"]].permute(2, 0, 1).unsqueeze(0).double()
    if c.get("gate"):
        x = x[:, :c["cin"]] * F.leaky_relu(x[:, c["cin"]:], CC.f32(c.get("in_slope", 0.1)))
    elif c.get("in_slope") is not None:
        x = in_lrelu(x) if in_lrelu else F.leaky_relu(x, CC.f32(c["in_slope"]))
    v = F.conv2d(x, t["w"].double(), t["bias"].double(), stride=c["s"], padding=g["pad"])
    if c.get("epi") == "clamp01":
        v = v if no_clamp else v.clamp(0, 1)
    elif c.get("epi") == "round":
        v = torch.sign(v) * torch.floor(v.abs() + 0.5) if half_away else torch.round(v)
    elif c.get("act") is not None:
        v = F.leaky_relu(v, CC.f32(c["act"]))
    sc = t["scale"].double() if t["scale"] is not None else None
    if scale_unshuffled:   # the scale applied per conv channel, before the shuffle
        v = v * sc[torch.arange(c["cout"]) % g["cy"]].view(1, -1, 1, 1)
        sc = None
    if c.get("shuf"):
        v = F.pixel_shuffle(v, 2)
    if t["res"] is not None:
        v = _nchw(t["res"][:, :, g["roff"]:g["roff"] + g["cy"]]) + v
    if t["res2"] is not None and not drop_res2:
        v = _nchw(t["res2"][:, :, g["r2off"]:g["r2off"] + g["cy"]]) + v
    if sc is not None:
        v = v * sc.view(1, -1, 1, 1)
    return v[0].permute(1, 2, 0)


def _nchw(hwc):
    return hwc.permute(2, 0, 1).unsqueeze(0).double()


def rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


SMALL = [
    C("small_gate_res", 24, 40, 1, 1, 9, 14, gate=True, nres=1, act=0.1, xoff=2, ypad=2),
    C("small_shuffle_scale", 10, 16, 3, 1, 7, 9, shuf=True, act=0.01),
    C("small_res2_in_slope_1p5", 6, 5, 3, 2, 11, 8, nres=2, in_slope=1.5, roff=2),
    C("small_res2_only_7x7_slope_1p5", 4, 3, 7, 1, 9, 9, res2_only=True, act=1.5, in_slope=-0.1),
]


@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_reference_agrees_with_torch(c):
    t = CC.tensors(c)
    assert t["scale"] is not None
    ref = CC.reference(c, t)
    assert ref.dtype == torch.float64
    assert rel(ref, formula(c, t)) < 1e-12


def test_strip_conv_is_the_whole_conv():
    """The row strips of the reference's convolution (large maps) give what one
    convolution gives, at both strides and an odd size."""
    g = torch.Generator().manual_seed(3)
    for k, s in ((3, 1), (3, 2), (7, 1), (1, 2), (5, 1)):
        x = torch.randn(1, 3, 37, 11, generator=g).double()
        w = torch.randn(4, 3, k, k, generator=g).double()
        whole = F.conv2d(x, w, stride=s, padding=(k - 1) // 2)
        assert rel(CC._conv64(x, w, s, (k - 1) // 2, rows=5), whole) < 1e-13


def test_bf16_reference_rounds_operands_after_the_input_op():
    c = C("small_bf16_in_lrelu", 8, 8, 3, 1, 6, 7, compute="bf16", in_slope=0.1)
    t = CC.tensors(c)
    x = t["x"].permute(2, 0, 1).unsqueeze(0)
    xin = F.leaky_relu(x, CC.f32(0.1)).bfloat16().double()      # fp32 op, then the rounding
    want = F.conv2d(xin, t["w"].bfloat16().double(), t["bias"].double(), padding=1)
    assert rel(CC.preact(c, t), want) < 1e-12
    assert rel(CC.preact(c, t), F.conv2d(x.double(), t["w"].double(), t["bias"].double(), padding=1)) > 1e-4


SENSITIVITY = [
    # (case, the deliberate error)
    ("edge_tconv_in_slope_1p5", dict(in_lrelu=lambda x: torch.maximum(x, x * 1.5))),
    ("edge_sconv_in_slope_1p5", dict(in_lrelu=lambda x: torch.maximum(x, x * 1.5))),
    ("xconv_3x3_32to32_res2", dict(drop_res2=True)),
    ("edge_sconv_res2_without_res", dict(drop_res2=True)),
    ("xconv_shuffle_64to64", dict(scale_unshuffled=True)),
    ("edge_sconv_act_clamp01", dict(no_clamp=True)),
    ("model_refine1_16to3_clamp", dict(no_clamp=True)),
]


@pytest.mark.parametrize("name,fault", SENSITIVITY, ids=[f"{n}-{list(f)[0]}" for n, f in SENSITIVITY])
def test_data_tells_the_error_apart(name, fault):
    c = BY_NAME[name]
    t = CC.tensors(c)
    ref = CC.reference(c, t)
    assert rel(formula(c, t), ref) < 1e-12
    assert rel(formula(c, t, **fault), ref) > 100 * BOUND[CC.compute_of(c)]


def test_round_is_half_to_even():
    """An exact tie (zero weights, bias 2.5) rounds to 2, where rounding half
    away from zero gives 3."""
    c = BY_NAME["edge_sconv_act_round"]
    t = CC.tensors(c)
    t["w"][0] = 0.0
    t["bias"][0] = 2.5
    ref = CC.reference(c, t)
    assert bool((ref[:, :, 0] == 2.0).all())
    assert rel(formula(c, t), ref) == 0.0
    assert bool((formula(c, t, half_away=True)[:, :, 0] == 3.0).all())


def _epi_cases(epi):
    return [c for c in CASES if c.get("epi") == epi]


@pytest.mark.parametrize("c", _epi_cases("clamp01"), ids=lambda c: c["name"])
def test_clamp_data_saturates_both_sides(c):
    lo, hi, inside = CC.clamp_shares(CC.preact(c, CC.tensors(c)))
    assert lo >= 0.02 and hi >= 0.02 and inside >= 0.5, (lo, hi, inside)


@pytest.mark.parametrize("c", _epi_cases("round"), ids=lambda c: c["name"])
def test_round_data_excludes_little(c):
    assert CC.compute_of(c) in ("f16x3", "f32")     # at bf16's bound the band would be 0.4 % wide
    assert not c.get("shuf") and CC.tensors(c)["scale"] is None   # integers, compared exactly
    pre = CC.preact(c, CC.tensors(c))
    assert CC.round_band(BOUND[CC.compute_of(c)], pre).double().mean().item() <= 1e-3
    assert pre.abs().max().item() > 8     # several integers each side


def test_every_case_has_a_conformance_parametrisation_and_a_route():
    from tests import test_gpu_conv_conformance as T
    mark = [m for m in T.test_conv_conformance.pytestmark if m.name == "parametrize"][0]
    names = sorted(c["name"] for c in CASES)
    assert sorted(c["name"] for c in mark.args[1]) == names
    assert sorted(mark.kwargs["ids"]) == names
    assert T.BOUND == BOUND
    assert any(m.name == "gpu" for m in ([T.pytestmark] if not isinstance(T.pytestmark, list) else T.pytestmark))
    assert sorted(CC.golden()) == names


def test_new_edges_sit_on_every_family():
    names = {c["name"] for c in CASES}
    for f, _ in CC.FAMILY:
        for e in ("in_slope_1p5", "in_slope_1", "slope_0", "slope_1", "act_clamp01", "act_round"):
            assert f"edge_{f}_{e}" in names
    assert {"edge_dconv_1x1_gate_in_slope_1p5", "edge_sgemm_gate_in_slope_1p5"} <= names
    for c in CASES:
        if c["name"].startswith("model_"):
            assert c["H"] * c["W"] <= 32 * 48 and c.get("ydt", c.get("dt", "f32")) == "f32"
            if c.get("epi") == "round":
                assert c["act"] == 0.01 and c["s"] == 2 and c["k"] == 3

"""Values of every pinned dcvc_conv2d call, at the kernel its route pins.

tests/test_gpu_conv_routing.py pins which kernel takes each call of
tests/conv_cases.py, on zeros; the family tests check values on the views and
slopes their authors picked.  Here every case of the same table runs once on
random data (non-zero bias, per-channel scale, random channels around offset
views) and must

  - take the route tests/golden/conv_routing.json records for it (so the
    values below are those of the pinned kernel; a route never depends on
    data), or raise the recorded error and leave the output untouched;
  - match conv_cases.reference(), the fp64 restatement of the ABI's formula,
    within the project's bound for the compute mode (below);
  - leave every channel of the output buffer outside y's window as it was.

ACT_ROUND cases compare the integers exactly, except where the fp64
pre-round value lies within bound * max|pre-round| of a half-integer (at most
0.1 % of the elements, asserted); ACT_CLAMP01 cases must saturate at least 2 %
of the reference's elements on each side and keep at least half inside.

Measured on an MI355X when the test was written (257 cases: 237 f16x3, 15
bf16, 5 f32; 9 of them pinned refusals): the largest error was 0.20 of the
bound for f16x3 (xconv_3x3_192to32_res0), 0.04 for f32, 0.003 for bf16; the 12
round cases excluded at most 0.037 % of their elements and had no other
element wrong; the 15 clamp cases saturated 2.7 - 12.8 % per side.  Before
tconv.hip refused input slopes above 1, edge_tconv_in_slope_1p5 ran on
tconv_ci_kernel<3, 1, 2, true> with an error of 0.31 of max|ref|.

DCVC_CONFORMANCE_LOG=<file> appends one line of figures per case.
"""
import os

import pytest
import torch

from tests.conv_cases import CASES, SENTINEL, clamp_shares, compute_of, golden, launch, preact, reference, round_band
from tests.test_gpu_kernels import TOL_BF16, bf16_err
from tests.test_gpu_sconv import TOL as TOL_F16X3

pytestmark = pytest.mark.gpu

# relative to max|ref|, the project's own bounds: f16x3 TOL of test_gpu_sconv.py
# / test_gpu_xconv.py (4e-6); f32 the 2e-5 of test_gpu_kernels.py's docstring;
# bf16 TOL_BF16 of test_gpu_kernels.py (1e-4) against fp64 of the bf16-rounded
# operands, through bf16_err for a bf16 output
BOUND = {"f16x3": TOL_F16X3, "f32": 2e-5, "bf16": TOL_BF16}
LOG = os.environ.get("DCVC_CONFORMANCE_LOG")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def log(c, **figures):
    line = c["name"] + " " + compute_of(c) + " " + " ".join(f"{k}={v}" for k, v in figures.items())
    print(line)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_conv_conformance(c):
    want = golden()[c["name"]]
    got, t = launch(c, "random")
    out = t["ybuf"].buf.cpu()
    cy = t["ybuf"].C - c.get("ypad", 0)
    assert got == want
    if want.startswith("error:"):
        assert bool((out == SENTINEL).all())
        return
    # nothing outside the view
    assert bool((out[:, :, cy:] == SENTINEL).all())
    y = out[:, :, :cy].double()
    bound = BOUND[compute_of(c)]
    pre = preact(c, t)
    ref = reference(c, t, pre)
    assert ref.shape == y.shape
    mag = ref.abs().max().item()
    if c.get("epi") == "round":
        # a pre-round value this close to a half-integer may round either way
        # within the compute mode's bound
        assert not c.get("shuf")
        near = round_band(bound, pre)[0].permute(1, 2, 0)
        share = near.double().mean().item()
        wrong = int(((y != ref) & ~near).sum())
        log(c, route=repr(got), excluded=f"{share:.3e}", wrong=wrong, span=f"{mag:.1f}")
        assert share <= 1e-3
        assert wrong == 0
        assert bool(((y - ref).abs() <= 1.0).all())      # inside the band: the neighbouring integer at most
        return
    if c.get("epi") == "clamp01":
        lo, hi, inside = clamp_shares(pre)
        log(c, sat_lo=f"{lo:.4f}", sat_hi=f"{hi:.4f}", inside=f"{inside:.4f}")
        assert lo >= 0.02 and hi >= 0.02 and inside >= 0.5
    if out.dtype == torch.bfloat16:
        err = bf16_err(y, ref)
    else:
        err = (y - ref).abs().max().item() / (mag + 1e-12)
    log(c, route=repr(got), err=f"{err:.3e}", of_bound=f"{err / bound:.3f}")
    assert err < bound, (err, bound)


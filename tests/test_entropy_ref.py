"""Pins tests/entropy_ref.py, the per-element reference that
tests/test_gpu_entropy_kernels.py holds the HIP kernels to, against the CPU
oracle, at every shape and on every input the GPU tests use.

Symbols, y_hat and scales are torch.equal to the oracle's mask-tensor
algebra.  The estimate-mode bits are where fp32 and fp64 differ: K (see
entropy_ref.bits_K) measures the fp32 oracle's error against the fp64
reference in units of 2^-24 of probability.  Measured with the CPU build of
torch used for development: K_cpu = 1.38 (Laplace), 1.34 (Normal, sigma >=
1e-5), 1.38 (Normal, sigma >= 0.11), 2.02 (factorized).  The GPU tests allow
the kernels 4 x the K_cpu measured on the machine they run on.
"""
import functools

import numpy as np
import pytest
import torch

from tests import entropy_ref as R

K_CPU_MAX = 4.0


def t4(a):
    """(C, H, W) numpy -> (1, C, H, W) torch."""
    return torch.from_numpy(np.ascontiguousarray(a))[None]


def same(t, a):
    return torch.equal(t.reshape(-1), torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))


def oracle_quadtree(case):
    """four_part_prior with the adaptor + spatial prior replaced by the case's
    fixed tensors (as tests/test_gpu_kernels.py does); also returns the
    y_hat_so_far each spatial-prior call was given."""
    from oracle import dc_oracle as O
    C = case["y"].shape[0]
    seen, it = [], iter(case["sms"])

    def spatial(x):
        seen.append(x[:, :C].clone())
        return t4(next(it))

    orig = O.conv
    O.conv = lambda P, name, x, stride=1, groups=1: x
    try:
        sym_w, sc_w, _, y_hat, _ = O.four_part_prior(None, t4(case["y"]), t4(case["params"]), ["a", "b", "c"], spatial)
    finally:
        O.conv = orig
    return sym_w, sc_w, y_hat, seen


@pytest.mark.parametrize("shape", R.QT_SHAPES)
@pytest.mark.parametrize("est", [False, True])
def test_quadtree_reference_equals_oracle(shape, est):
    from oracle import dc_oracle as O
    case = R.quadtree_case(*shape, est=est)
    steps, so_far, yhat = R.quadtree_run(case["params"], case["sms"], y=case["y"])
    sym_w, sc_w, y_hat, seen = oracle_quadtree(case)
    for k in range(4):
        assert same(sym_w[k], steps[k]["sym_f"]), k
        assert same(sc_w[k], steps[k]["scale"]), k
        if k < 3:
            assert same(seen[k], so_far[k]), k
    assert same(y_hat, yhat)
    # the engineered inputs are there: both sides of the quant_step clamp,
    # exact ties, symbols beyond the int16 clamp
    qs_raw = case["params"][:shape[0]]
    assert (qs_raw < 0.5).any() and (qs_raw == 0.5).any() and (qs_raw > 0.5).any()
    allsym = np.concatenate([s["sym_f"].reshape(-1) for s in steps])
    assert (np.abs(allsym) > 30000).any() and (allsym == 30000).any()

    # decoder: the oracle's decompress fed the clamped symbols
    syms = [s["sym"] for s in steps]
    dsteps, _, dyhat = R.quadtree_run(case["params"], case["sms"], syms=syms)
    it, calls = iter(case["sms"]), []

    def decode(scales_r):
        k = len(calls)
        calls.append(scales_r)
        return t4(syms[k])

    orig = O.conv
    O.conv = lambda P, name, x, stride=1, groups=1: x
    try:
        d = O.four_part_decompress(None, t4(case["params"]), ["a", "b", "c"], lambda x: t4(next(it)), decode)
    finally:
        O.conv = orig
    assert same(d, dyhat)
    for k in range(4):
        assert same(calls[k], dsteps[k]["scale"]), k
        inr = np.abs(steps[k]["sym_f"]) <= 30000
        assert np.array_equal(dsteps[k]["yhs"][inr], steps[k]["yhs"][inr])


def test_quadtree_ties_round_half_to_even():
    case = R.quadtree_case(*R.QT_SHAPES[2])
    ties = 0
    for s in R.quadtree_run(case["params"], case["sms"], y=case["y"])[0]:
        res = (R.gather(case["y"], s["ch"]) / s["qs"] - s["mean"]).astype(np.float64)
        t = (np.abs(res - np.floor(res) - 0.5) == 0) & (np.abs(res) < 100)
        ties += int(t.sum())
        assert (s["sym_f"][t] % 2 == 0).all()
    assert ties >= 50


@pytest.mark.parametrize("shape", R.DP_SHAPES)
@pytest.mark.parametrize("est", [False, True])
def test_dual_reference_equals_oracle(shape, est):
    from oracle import hem_oracle as O
    case = R.dual_case(*shape, est=est)
    C = shape[0]
    buf, post = case["buf"], case["post"]
    means, scales, qs = t4(buf[C:2 * C]), t4(buf[2 * C:3 * C]), t4(buf[3 * C:])
    steps, buf1, yhat = R.dual_run(buf, case["sm"], y=case["y"])
    seen = []

    def spatial(x):
        seen.append(x.clone())
        return t4(case["sm"])

    q0, q1, s0, s1, y_hat = O.dual_prior(None, t4(case["y"]), means, scales, qs, spatial, write=True)
    assert same(q0, steps[0]["sym_f"]) and same(q1, steps[1]["sym_f"])
    assert same(s0, steps[0]["scale"]) and same(s1, steps[1]["scale"])
    assert same(seen[0], buf1)          # the whole spatial-prior input, rewritten sections included
    assert same(y_hat, yhat)
    assert same(y_hat * torch.from_numpy(post)[None, :, None, None], R.dual_run(buf, case["sm"], y=case["y"], post=post)[2])
    allsym = np.concatenate([s["sym_f"].reshape(-1) for s in steps])
    if shape != R.DP_SHAPES[0]:         # 16 elements do not hold every engineered value
        assert (np.abs(allsym) >= 1e6 - 3).any() and (np.abs(allsym) > 2 ** 15).any()
    assert (buf[3 * C:] < 0.5).any() and (buf1[3 * C:] >= 0.5).all()

    syms = [s["sym_f"] for s in steps]
    _, dbuf1, dyhat = R.dual_run(buf, case["sm"], syms=syms)
    it = iter(syms)
    seen.clear()
    d = O.dual_decompress(None, means, scales, qs, spatial, lambda s: t4(next(it)))
    assert same(d, dyhat) and same(seen[0], dbuf1)
    # int32 symbols are not clamped: the decoder reproduces the encoder everywhere
    assert np.array_equal(dbuf1, buf1) and np.array_equal(dyhat, yhat)


def index_sites(kind, est=False):
    """Every scale that an index is computed from in the GPU tests."""
    out = []
    if kind == "quadtree":
        for shape in R.QT_SHAPES:
            c = R.quadtree_case(*shape, est=est)
            out += [s["scale"].reshape(-1) for s in R.quadtree_run(c["params"], c["sms"], y=c["y"])[0]]
    else:
        for shape in R.DP_SHAPES:
            c = R.dual_case(*shape, est=est)
            out += [s["scale"].reshape(-1) for s in R.dual_run(c["buf"], c["sm"], y=c["y"])[0]]
    return np.concatenate(out)


@pytest.mark.parametrize("kind,table", [("quadtree", R.LAPLACE_TABLE), ("dual", R.NORMAL_TABLE)])
def test_indexes_equal_oracle_away_from_integers(kind, table):
    from oracle import dc_oracle as O
    sc = index_sites(kind)
    v = R.index_float64(sc, *table)
    near = R.near_integer(v, R.IDX_TIE_EPS)
    print(f"{kind}: near-integer share {near.mean():.4%} of {near.size}")
    assert near.mean() <= R.IDX_TIE_SHARE
    got = O.build_indexes(torch.from_numpy(sc), *table).numpy().astype(np.int64)
    ref = R.index_of(v)
    assert np.array_equal(got[~near], ref[~near])
    assert (np.abs(got - ref)[near] <= 1).all()
    # scales that are 0, negative or below 1e-5 index 0; above the table's top, 255
    assert (ref[sc <= 1e-5] == 0).all() and (sc <= 0).any()
    assert (ref[sc > 64.0] == 255).all() and (sc == np.float32(1e12)).any()


@functools.lru_cache(maxsize=None)
def k_cpu():
    """K of the fp32 oracle's bits against the fp64 reference, per
    distribution, on the GPU tests' inputs."""
    from oracle import dc_oracle as DC, hem_oracle as HEM
    out = {}
    yq, sg = R.estimate_pairs("quadtree")
    ty, ts = torch.from_numpy(yq), torch.from_numpy(sg)
    out["laplace"] = R.bits_K(DC.laplace_bits(ty, ts).numpy(), R.laplace_prob(yq, sg, 1e-5))
    out["normal_dc"] = R.bits_K(DC.gaussian_bits(ty, ts).numpy(), R.normal_prob(yq, sg, 1e-5))
    yq, sg = R.estimate_pairs("dual")
    ty, ts = torch.from_numpy(yq), torch.from_numpy(sg)
    out["normal_hem"] = R.bits_K(HEM.gaussian_bits(ty, ts).numpy(), R.normal_prob(yq, sg, 0.11))
    out["laplace"] = max(out["laplace"], R.bits_K(DC.laplace_bits(ty, ts).numpy(), R.laplace_prob(yq, sg, 1e-5)))
    kz = 0.0
    for shape in R.FACTORIZED_SHAPES:
        c = R.factorized_case(*shape)
        P = {"be." + n: v.reshape(1, -1, 1, 1) for n, v in c["raw"].items()}
        kz = max(kz, R.bits_K(DC.z_bits(P, "be", t4(c["z"])).numpy(), R.factorized_prob(c["z"], c["table"])))
    out["factorized"] = kz
    return out


def test_oracle_bits_within_K_of_fp64():
    k = k_cpu()
    print("K_cpu", {n: round(v, 3) for n, v in k.items()})
    for name, v in k.items():
        assert 0.0 < v <= K_CPU_MAX, (name, v)


def test_bits_inputs_reach_both_clamps_and_totals_agree():
    from oracle import dc_oracle as DC, hem_oracle as HEM
    for kind, fn, prob, smin in (("quadtree", DC.laplace_bits, R.laplace_prob, 1e-5),
                                 ("quadtree", DC.gaussian_bits, R.normal_prob, 1e-5),
                                 ("dual", HEM.gaussian_bits, R.normal_prob, 0.11)):
        yq, sg = R.estimate_pairs(kind)
        ref = R.probs_to_bits(prob(yq, sg, smin))
        assert (ref == 0).any() and (ref > 16.6).any() and ref.max() < 16.61
        got = fn(torch.from_numpy(yq), torch.from_numpy(sg)).double().numpy()
        assert abs(got.sum() - ref.sum()) <= 1e-5 * ref.sum()
    # the sigma clamp matters on these inputs: the other bound gives other bits
    yq, sg = R.estimate_pairs("dual")
    pa = R.normal_prob(yq, sg, 0.11)
    a, b = R.probs_to_bits(pa), R.probs_to_bits(R.normal_prob(yq, sg, 1e-5))
    assert (np.abs(a - b) > 4 * R.bits_bound(pa, 4 * k_cpu()["normal_hem"])).any()

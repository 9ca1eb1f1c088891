"""The quadtree, dual-prior, bit-estimate and symbol-transpose kernels of
misc.hip / hem.hip, each against tests/entropy_ref.py (a per-element fp32 /
fp64 reference that tests/test_entropy_ref.py pins to the CPU oracle).

Symbols, y_hat and the rewritten spatial-prior sections are compared bit for
bit: the arithmetic is one correctly rounded divide, a subtract, rint, an add
and one or two multiplies, so a fast-math flag or a reciprocal-multiply shows.
Every output lives in a channel window of a wider, sentinel-filled buffer and
the whole buffer is compared, so a store outside the step's own (pixel,
channel) sites shows too.  Indexes equal clamp(trunc(index_float64)) except
within IDX_TIE_EPS of an integer.  Decoder-side kernels must reproduce the
encoder-side kernels' indexes and y_hat exactly.

Estimate-mode bits are held per element to
    |dbits| <= K_gpu 2^-24 / ((p + 1e-5) ln2) + 2^-20,   K_gpu = 4 K_cpu,
with K_cpu the fp32 CPU oracle's own error against the fp64 reference on the
same inputs (tests/test_entropy_ref.py:k_cpu; where measured: Laplace 1.38,
Normal 1.34 with sigma >= 1e-5 and 1.38 with sigma >= 0.11, factorized 2.02),
and each call's total to 1e-5 relative of the fp64 total.

Observed on an MI355X (K as entropy_ref.bits_K, the largest over all calls):
Laplace 0.01, Normal 0.33 (sigma >= 1e-5) and 0.60 (sigma >= 0.11),
factorized 2.02; totals within 9e-8 (factorized 8.1e-6).  The Laplace and
Normal kernels first computed cdf(y + 0.5) - cdf(y - 0.5) literally, as the
fp32 oracle does: K 1.37 / 1.16 / 1.23, like the oracle's, but the totals of
the 8-element calls of the smallest shapes missed 1e-5 (up to 5.4e-5, the
oracle likewise): one fp32 rounding of a CDF next to 1 is 9e-3 bits at
p ~ 1e-5.  bin_prob() in misc.hip / hem.hip now evaluates the same
probability where nothing cancels.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import entropy_ref as R

pytestmark = pytest.mark.gpu

SENT = -777.125          # sentinel every output buffer starts with
PAD = 32                 # sentinel tail of the flat symbol / index / bits buffers


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """A GPU error poisons the process: end the session, launch nothing more."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, stopping: {e}", returncode=3)


def K():
    from dcvc_amd import hip
    return hip


def k_gpu(name):
    from tests.test_entropy_ref import k_cpu
    return 4.0 * k_cpu()[name]


def dev(a):
    """(C, H, W) numpy -> (H, W, C) device tensor."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).transpose(1, 2, 0))).cuda()


def host(t):
    """(H, W, C) device tensor -> (C, H, W) numpy."""
    return np.ascontiguousarray(t.detach().float().cpu().numpy().transpose(2, 0, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def window(C, H, W, off, extra, data=None, dtype=torch.float32):
    """Act over channels [off, off + C) of a sentinel-filled (H, W, C + extra)
    buffer; ``data`` (C, H, W) fills the window."""
    buf = torch.full((H, W, C + extra), SENT, dtype=dtype, device="cuda")
    if data is not None:
        buf[:, :, off:off + C] = dev(data).to(dtype)
    return K().Act(buf).ch(off, C)


def flat(n, dtype):
    return torch.full((n + PAD,), -99, dtype=dtype, device="cuda")


def tail_intact(t, n):
    return bool((t[n:] == -99).all())


def check_indexes(got, ref_v):
    """got == clamp(trunc(v)) except within IDX_TIE_EPS of an integer (+-1)."""
    ref, near = R.index_of(ref_v), R.near_integer(ref_v, R.IDX_TIE_EPS)
    d = np.asarray(got, np.int64) - ref
    assert (d[~near] == 0).all(), (np.flatnonzero((d != 0) & ~near)[:8], d[(d != 0) & ~near][:8])
    assert (np.abs(d[near]) <= 1).all()


def check_bits(got, p, name, what):
    """The per-element bound."""
    got, p = np.asarray(got, np.float64).reshape(-1), np.asarray(p, np.float64).reshape(-1)
    ref = R.probs_to_bits(p)
    kg = k_gpu(name)
    print(f"K_gpu_observed {what} {name} {R.bits_K(got, p):.3f} (allowed {kg:.3f})")
    bad = np.abs(got - ref) > R.bits_bound(p, kg)
    assert not bad.any(), (what, np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8], p[bad][:8])


BITS_REL = 1e-5          # a call's bit total against the fp64 total (tests/test_gpu_model_dc.py)


def total_rel(got, p, what):
    """|total - fp64 total| / fp64 total of one call."""
    got, ref = np.asarray(got, np.float64).sum(), R.probs_to_bits(p).sum()
    print(f"bits_rel {what} {abs(got - ref) / ref:.2e}")
    return abs(got - ref) / ref


# ------------------------------------------------------------------ quadtree
class QtBufs:
    """The production layout: params at ch(C, 3C) and y_hat_so_far at ch(0, C)
    of the spatial-prior buffer; y_hat in a window at an odd channel offset."""

    def __init__(self, case):
        h = K()
        self.C, self.H, self.W = C, H, W = case["y"].shape
        self.sp = torch.full((H, W, 4 * C), SENT, device="cuda")
        self.sp[:, :, C:] = dev(case["params"])
        self.yhs, self.params = h.Act(self.sp).ch(0, C), h.Act(self.sp).ch(C, 3 * C)
        self.yhat = window(C, H, W, 3, 5)
        self.y = window(C, H, W, 1, 2, case["y"])
        self.sms = [window(2 * C, H, W, 1, 3, sm) for sm in case["sms"]]
        self.n = C // 4 * H * W
        self.exp_sp = np.concatenate([np.full((C, H, W), SENT, np.float32), case["params"]])
        self.exp_wide = np.full((C + 5, H, W), SENT, np.float32)

    def sm(self, k):
        return None if k == 0 else self.sms[k - 1]

    def expect(self, step):
        R.scatter(self.exp_sp, step["ch"], step["yhs"])
        R.scatter(self.exp_wide, step["ch"] + 3, step["yhat"])

    def check(self, what):
        torch.cuda.synchronize()
        assert same_bits(host(self.sp), self.exp_sp), what
        assert same_bits(host(self.yhat.buf), self.exp_wide), what


def near_share(steps, table):
    v = np.concatenate([R.index_float64(s["scale"].reshape(-1), *table) for s in steps])
    return R.near_integer(v, R.IDX_TIE_EPS).mean()


@pytest.mark.parametrize("shape", R.QT_SHAPES)
def test_quadtree_encode_index_decode_steps(shape):
    h = K()
    case = R.quadtree_case(*shape)
    steps, _, _ = R.quadtree_run(case["params"], case["sms"], y=case["y"])
    log_min, log_step = R.LAPLACE_TABLE
    assert near_share(steps, R.LAPLACE_TABLE) <= R.IDX_TIE_SHARE   # from the reference alone
    enc, dec = QtBufs(case), QtBufs(case)
    n = enc.n
    syms = []
    for k in range(4):
        sym, idx, idx2 = flat(n, torch.int16), flat(n, torch.int16), flat(n, torch.int16)
        h.qt_encode_step(enc.y, enc.params, enc.sm(k), k, enc.yhs, enc.yhat, sym, idx, log_min, log_step)
        h.qt_indexes_step(dec.params, dec.sm(k), k, idx2, log_min, log_step)
        enc.expect(steps[k])
        enc.check(("encode", k))
        assert tail_intact(sym, n) and tail_intact(idx, n) and tail_intact(idx2, n)
        assert np.array_equal(sym[:n].cpu().numpy(), steps[k]["sym"].reshape(-1).astype(np.int16)), k
        check_indexes(idx[:n].cpu().numpy(), R.index_float64(steps[k]["scale"].reshape(-1), log_min, log_step))
        assert torch.equal(idx2, idx), k           # decoder-side indexes: no tolerance
        syms.append(sym)
    # decoder fed the encoder's symbols, all steps in order
    dsteps, _, _ = R.quadtree_run(case["params"], case["sms"], syms=[s["sym"] for s in steps])
    for k in range(4):
        h.qt_decode_step(dec.params, dec.sm(k), k, syms[k], dec.yhs, dec.yhat)
        dec.expect(dsteps[k])
        dec.check(("decode", k))
    # ... reproduces the encoder's y_hat, except where the int16 clamp cut the symbol
    e_sp, d_sp, e_w, d_w = host(enc.sp), host(dec.sp), host(enc.yhat.buf), host(dec.yhat.buf)
    inr = np.ones(case["y"].shape, bool)
    for s in steps:
        R.scatter(inr, s["ch"], np.abs(s["sym_f"]) <= 30000)
    assert not inr.all()
    C = shape[0]
    assert same_bits(e_sp[:C][inr], d_sp[:C][inr]) and same_bits(e_w[3:3 + C][inr], d_w[3:3 + C][inr])


@functools.lru_cache(maxsize=None)
def run_quadtree_estimate(shape, gaussian):
    """The four estimate steps next to the four encode steps on twin buffers;
    y_hat is checked here, the bits are returned: [(bits, p)] per step."""
    h = K()
    case = R.quadtree_case(*shape, est=True)
    steps, _, _ = R.quadtree_run(case["params"], case["sms"], y=case["y"])
    enc, est = QtBufs(case), QtBufs(case)
    n = enc.n
    prob = R.normal_prob if gaussian else R.laplace_prob
    out = []
    for k in range(4):
        sym, idx, bits = flat(n, torch.int16), flat(n, torch.int16), flat(n, torch.float32)
        h.qt_encode_step(enc.y, enc.params, enc.sm(k), k, enc.yhs, enc.yhat, sym, idx, *R.LAPLACE_TABLE)
        h.qt_estimate_step(est.y, est.params, est.sm(k), k, est.yhs, est.yhat, bits, gaussian)
        enc.expect(steps[k])
        est.expect(steps[k])
        enc.check(("encode", k))
        est.check(("estimate", k))
        assert same_bits(host(est.sp), host(enc.sp)) and same_bits(host(est.yhat.buf), host(enc.yhat.buf))
        assert tail_intact(bits, n)
        out.append((bits[:n].cpu().numpy(), prob(steps[k]["sym_f"], steps[k]["scale"], 1e-5).reshape(-1)))
    return out


@pytest.mark.parametrize("shape", R.QT_SHAPES)
@pytest.mark.parametrize("gaussian", [0, 1])
def test_quadtree_estimate_steps(shape, gaussian):
    """y_hat outputs bit-equal to the encode step's; every element's bits
    within the K_gpu bound of the fp64 reference."""
    res = run_quadtree_estimate(shape, gaussian)
    for k, (got, p) in enumerate(res):
        check_bits(got, p, "normal_dc" if gaussian else "laplace", f"quadtree{shape} step {k}")
    if shape == R.QT_SHAPES[2]:
        ref = R.probs_to_bits(np.concatenate([p for _, p in res]))
        assert (ref == 0).any() and (ref > 16.6).any()   # p -> 1 and p -> 0


@pytest.mark.parametrize("shape", R.QT_SHAPES)
@pytest.mark.parametrize("gaussian", [0, 1])
def test_quadtree_estimate_call_totals(shape, gaussian):
    """Each call's bit total within 1e-5 relative of the fp64 total."""
    rel = [total_rel(got, p, f"quadtree{shape} {'normal' if gaussian else 'laplace'} step {k}")
           for k, (got, p) in enumerate(run_quadtree_estimate(shape, gaussian))]
    assert max(rel) <= BITS_REL, rel


# ---------------------------------------------------------------- dual prior
class DpBufs:
    def __init__(self, case, post):
        self.C, self.H, self.W = C, H, W = case["y"].shape
        self.buf = window(4 * C, H, W, 1, 2, case["buf"])
        self.yhat = window(C, H, W, 3, 5)
        self.y = window(C, H, W, 1, 2, case["y"])
        self.sm_act = window(2 * C, H, W, 1, 3, case["sm"])
        self.post = torch.from_numpy(case["post"]).cuda() if post else None
        self.n = C // 2 * H * W
        self.exp_buf = np.full((4 * C + 2, H, W), SENT, np.float32)
        self.exp_buf[1:1 + 4 * C] = case["buf"]
        self.exp_wide = np.full((C + 5, H, W), SENT, np.float32)

    def sm(self, k):
        return None if k == 0 else self.sm_act

    def expect(self, step):
        if "buf" in step:
            self.exp_buf[1:1 + 4 * self.C] = step["buf"]
        R.scatter(self.exp_wide, step["ch"] + 3, step["yhat"])

    def check(self, what):
        torch.cuda.synchronize()
        assert same_bits(host(self.buf.buf), self.exp_buf), what
        assert same_bits(host(self.yhat.buf), self.exp_wide), what


@pytest.mark.parametrize("shape", R.DP_SHAPES)
@pytest.mark.parametrize("post", [False, True])
def test_dual_prior_encode_index_decode_steps(shape, post):
    h = K()
    case = R.dual_case(*shape)
    p = case["post"] if post else None
    steps, _, _ = R.dual_run(case["buf"], case["sm"], y=case["y"], post=p)
    log_min, log_step = R.NORMAL_TABLE
    assert near_share(steps, R.NORMAL_TABLE) <= R.IDX_TIE_SHARE
    enc, dec = DpBufs(case, post), DpBufs(case, post)
    n = enc.n
    for k in range(2):
        sym, idx, idx2 = flat(n, torch.int32), flat(n, torch.int16), flat(n, torch.int16)
        h.dp_encode_step(enc.y, enc.buf, enc.sm(k), k, enc.yhat, enc.post, sym, idx, log_min, log_step)
        # the decoder computes its indexes before it has the step's symbols
        h.dp_indexes_step(dec.buf, dec.sm(k), k, idx2, log_min, log_step)
        h.dp_decode_step(dec.buf, dec.sm(k), k, sym, dec.yhat, dec.post)
        enc.expect(steps[k])
        dec.expect(steps[k])
        enc.check(("encode", k))
        dec.check(("decode", k))
        assert tail_intact(sym, n) and tail_intact(idx, n) and tail_intact(idx2, n)
        assert np.array_equal(sym[:n].cpu().numpy(), steps[k]["sym_f"].reshape(-1).astype(np.int32)), k
        check_indexes(idx[:n].cpu().numpy(), R.index_float64(steps[k]["scale"].reshape(-1), log_min, log_step))
        assert torch.equal(idx2, idx), k
    assert same_bits(host(enc.buf.buf), host(dec.buf.buf)) and same_bits(host(enc.yhat.buf), host(dec.yhat.buf))


DP_DIST = {"normal_hem": (1, 0.11, R.normal_prob), "laplace": (0, 1e-5, R.laplace_prob)}


@functools.lru_cache(maxsize=None)
def run_dual_estimate(shape, dist):
    """As run_quadtree_estimate; the Normal case runs with post_scale."""
    h = K()
    case = R.dual_case(*shape, est=True)
    post = dist == "normal_hem"
    steps, _, _ = R.dual_run(case["buf"], case["sm"], y=case["y"], post=case["post"] if post else None)
    gaussian, smin, prob = DP_DIST[dist]
    enc, est = DpBufs(case, post), DpBufs(case, post)
    n = enc.n
    out = []
    for k in range(2):
        sym, idx, bits = flat(n, torch.int32), flat(n, torch.int16), flat(n, torch.float32)
        h.dp_encode_step(enc.y, enc.buf, enc.sm(k), k, enc.yhat, enc.post, sym, idx, *R.NORMAL_TABLE)
        h.dp_estimate_step(est.y, est.buf, est.sm(k), k, est.yhat, est.post, bits, gaussian, smin)
        enc.expect(steps[k])
        est.expect(steps[k])
        enc.check(("encode", k))
        est.check(("estimate", k))
        assert same_bits(host(est.buf.buf), host(enc.buf.buf)) and same_bits(host(est.yhat.buf), host(enc.yhat.buf))
        assert tail_intact(bits, n)
        out.append((bits[:n].cpu().numpy(), prob(steps[k]["sym_f"], steps[k]["scale"], smin).reshape(-1)))
    return out


@pytest.mark.parametrize("shape", R.DP_SHAPES)
@pytest.mark.parametrize("dist", ["normal_hem", "laplace"])
def test_dual_prior_estimate_steps(shape, dist):
    res = run_dual_estimate(shape, dist)
    for k, (got, p) in enumerate(res):
        check_bits(got, p, dist, f"dual{shape} step {k}")
    if shape == R.DP_SHAPES[2]:
        ref = R.probs_to_bits(np.concatenate([p for _, p in res]))
        assert (ref == 0).any() and (ref > 16.6).any()


@pytest.mark.parametrize("shape", R.DP_SHAPES)
@pytest.mark.parametrize("dist", ["normal_hem", "laplace"])
def test_dual_prior_estimate_call_totals(shape, dist):
    """Each call's bit total within 1e-5 relative of the fp64 total."""
    rel = [total_rel(got, p, f"dual{shape} {dist} step {k}") for k, (got, p) in enumerate(run_dual_estimate(shape, dist))]
    assert max(rel) <= BITS_REL, rel


# ------------------------------------------------------- factorized bits, sum
@pytest.mark.parametrize("shape", R.FACTORIZED_SHAPES)
def test_factorized_bits(shape):
    h = K()
    C, H, W = shape
    case = R.factorized_case(*shape)
    z = window(C, H, W, 3, 4, case["z"])
    n = C * H * W
    bits = flat(n, torch.float32)
    h.factorized_bits(z, torch.from_numpy(case["table"]).cuda(), bits)
    torch.cuda.synchronize()
    assert tail_intact(bits, n)
    p = R.factorized_prob(case["z"], case["table"]).transpose(1, 2, 0)   # the kernel's order: (pixel, channel)
    assert (R.probs_to_bits(p) > 16.6).any()                             # saturated sigmoids
    check_bits(bits[:n].cpu().numpy(), p, "factorized", f"factorized{shape}")
    assert total_rel(bits[:n].cpu().numpy(), p, f"factorized{shape}") <= BITS_REL


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 100003])
def test_sum_f32(n):
    h = K()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((3,), SENT, device="cuda")
    h.sum_f32(xd, out[0:1])
    h.sum_f32(xd, out[1:2])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert same_bits(o[0:1], o[1:2]) and o[2] == np.float32(SENT)
    # each thread's strided sum has ceil(n / 1024) terms, the tree 10 levels
    x64 = x.astype(np.float64)
    assert abs(float(o[0]) - x64.sum()) <= (math.ceil(n / 1024) + 10) * 2.0 ** -24 * np.abs(x64).sum()


# ---------------------------------------------------------- symbol transposes
TSHAPE = (5, 9, 13)      # 585 elements: three blocks, the last one partial


def _sym_values(limit, dtype):
    C, H, W = TSHAPE
    rng = np.random.default_rng(5)
    x = rng.integers(-limit, limit + 1, C * H * W).astype(np.float64)
    x[:8] = [limit, -limit, 0, 1, -1, 255, -256, 2]
    return x.astype(dtype).reshape(TSHAPE)


@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_nhwc_to_symbols_clamps(src):
    h = K()
    C, H, W = TSHAPE
    x = _sym_values(29000, np.float32)
    x.reshape(-1)[8:20] = [30000.4, 4e4, -1e9, -30000.6, 29999.9, -29999.9, 2.7, -2.7, 30000.0, -30000.0, 1e9, 0.9]
    dt = torch.float32 if src == "f32" else torch.bfloat16
    xa = window(C, H, W, 3, 6, x, dtype=dt)
    xin = host(xa.t())                                  # what the kernel reads (bf16-rounded)
    n = C * H * W
    sym = flat(n, torch.int16)
    h.to_symbols(xa, sym)
    torch.cuda.synchronize()
    assert tail_intact(sym, n)
    ref = np.trunc(np.clip(xin, -30000.0, 30000.0)).astype(np.int16).reshape(-1)   # NCHW order
    assert np.array_equal(sym[:n].cpu().numpy(), ref)
    assert (ref == 30000).any() and (ref == -30000).any()


@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_nhwc_to_symbols_i32_exact(src):
    h = K()
    C, H, W = TSHAPE
    x = _sym_values(2 ** 24 if src == "f32" else 256, np.float32)
    xa = window(C, H, W, 3, 6, x, dtype=torch.float32 if src == "f32" else torch.bfloat16)
    n = C * H * W
    sym = flat(n, torch.int32)
    h.to_symbols_i32(xa, sym)
    torch.cuda.synchronize()
    assert tail_intact(sym, n)
    assert np.array_equal(sym[:n].cpu().numpy(), x.reshape(-1).astype(np.int32))


@pytest.mark.parametrize("dst", ["f32", "bf16"])
@pytest.mark.parametrize("wide", [False, True])
def test_symbols_to_nhwc_inverse(dst, wide):
    h = K()
    C, H, W = TSHAPE
    limit = 256 if dst == "bf16" else (2 ** 24 if wide else 30000)
    v = _sym_values(limit, np.int32 if wide else np.int16)
    sym = torch.from_numpy(v.reshape(-1)).cuda()
    dt = torch.float32 if dst == "f32" else torch.bfloat16
    ya = window(C, H, W, 3, 6, dtype=dt)
    (h.from_symbols_i32 if wide else h.from_symbols)(sym, ya)
    torch.cuda.synchronize()
    exp = np.full((C + 6, H, W), SENT, np.float32)
    exp = host(torch.from_numpy(exp.transpose(1, 2, 0)).to(dt))   # the sentinel as dst holds it
    exp[3:3 + C] = v.astype(np.float32)
    assert same_bits(host(ya.buf), exp)
    # and back
    back = flat(C * H * W, torch.int32 if wide else torch.int16)
    (h.to_symbols_i32 if wide else h.to_symbols)(ya, back)
    torch.cuda.synchronize()
    assert torch.equal(back[:C * H * W], sym)


@pytest.mark.parametrize("dst", ["f32", "bf16"])
def test_fill_window(dst):
    h = K()
    C, H, W = TSHAPE
    dt = torch.float32 if dst == "f32" else torch.bfloat16
    ya = window(C, H, W, 3, 6, dtype=dt)
    h.fill(ya, 1.5)
    torch.cuda.synchronize()
    exp = host(torch.full((H, W, C + 6), SENT).to(dt))
    exp[3:3 + C] = 1.5
    assert same_bits(host(ya.buf), exp)


@pytest.mark.parametrize("in_place", [False, True])
def test_channel_div_is_a_true_division(in_place):
    h = K()
    C, H, W = TSHAPE
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(TSHAPE) * 7).astype(np.float32)
    q = rng.uniform(0.5, 3.0, C).astype(np.float32)
    ref = x / q[:, None, None]
    assert not same_bits(ref, x * (np.float32(1) / q)[:, None, None])   # a reciprocal-multiply would differ here
    xa = window(C, H, W, 1, 4, x)
    ya = xa if in_place else window(C, H, W, 3, 6)
    h.channel_div(xa, torch.from_numpy(q).cuda(), ya)
    torch.cuda.synchronize()
    exp = np.full((C + (4 if in_place else 6), H, W), SENT, np.float32)
    off = 1 if in_place else 3
    exp[off:off + C] = ref
    assert same_bits(host(ya.buf), exp)
    if not in_place:
        assert same_bits(host(xa.t()), x)


# ------------------------------------------------------------ host validation
class Described:
    """A tensor descriptor that differs from the memory behind it only in what
    it claims (here: the dtype), over a buffer that is large enough either way."""

    def __init__(self, act, dtype):
        c = act.c()
        self._c = K().CTensor(c.ptr, dtype, c.H, c.W, c.C, c.cstride, c.coff)

    def c(self):
        return self._c


def invalid(fn, *args):
    from dcvc_amd._native import NativeError
    with pytest.raises(NativeError, match="invalid argument"):
        fn(*args)
    torch.cuda.synchronize()


def act(C, H, W):
    return window(C, H, W, 0, 0)


def test_quadtree_host_validation():
    """Every mismatched tensor is LARGER than the call needs, so a call that
    slipped through validation would still stay inside every buffer."""
    h = K()
    C, H, W = 8, 4, 6
    y, params, sm, yhs, yhat = act(C, H, W), act(3 * C, H, W), act(2 * C, H, W), act(C, H, W), act(C, H, W)
    n = (C + 4) // 4 * (H + 1) * (W + 1)
    sym, idx, bits = flat(n, torch.int16), flat(n, torch.int16), flat(n, torch.float32)
    lm, ls = R.LAPLACE_TABLE

    def enc(y=y, params=params, sm=None, k=0, yhs=yhs, yhat=yhat):
        h.qt_encode_step(y, params, sm, k, yhs, yhat, sym, idx, lm, ls)

    def est(y=y, params=params, sm=None, k=0, yhs=yhs, yhat=yhat):
        h.qt_estimate_step(y, params, sm, k, yhs, yhat, bits, 0)

    def dec(params=params, sm=None, k=0, yhs=yhs, yhat=yhat):
        h.qt_decode_step(params, sm, k, sym, yhs, yhat)

    def ind(params=params, sm=None, k=0):
        h.qt_indexes_step(params, sm, k, idx, lm, ls)

    enc(), est(), dec(), ind(), enc(sm=sm, k=1), est(sm=sm, k=3), dec(sm=sm, k=2), ind(sm=sm, k=1)   # the valid calls
    torch.cuda.synchronize()
    taller, wider = (lambda c: act(c, H + 1, W)), (lambda c: act(c, H, W + 1))
    for f in (enc, est, dec, ind):
        invalid(lambda: f(k=-1))
        invalid(lambda: f(k=4, sm=sm))
        invalid(lambda: f(k=0, sm=sm))                        # sm present at k = 0
        invalid(lambda: f(k=1))                               # sm absent at k > 0
        invalid(lambda: f(params=act(3 * C + 1, H, W)))       # wrong params channel count
        invalid(lambda: f(params=Described(params, h.BF16)))  # bf16 params
        invalid(lambda: f(k=1, sm=act(2 * C + 1, H, W)))
        invalid(lambda: f(k=1, sm=taller(2 * C)))
        invalid(lambda: f(k=1, sm=wider(2 * C)))
    # C not a multiple of 4
    y6, p6, o6 = act(6, H, W), act(18, H, W), act(6, H, W)
    invalid(lambda: enc(y=y6, params=p6, yhs=o6, yhat=o6))
    invalid(lambda: est(y=y6, params=p6, yhs=o6, yhat=o6))
    invalid(lambda: dec(params=p6, yhs=o6, yhat=o6))
    invalid(lambda: ind(params=p6))
    for f in (enc, est, dec):
        for big in (taller, wider):
            invalid(lambda: f(yhs=big(C)))
            invalid(lambda: f(yhat=big(C)))
        invalid(lambda: f(yhs=act(C + 1, H, W)))
        invalid(lambda: f(yhat=act(C + 1, H, W)))
    for f in (enc, est):
        for big in (taller, wider):
            invalid(lambda: f(params=big(3 * C)))
            # y smaller than all the rest
            invalid(lambda: f(params=big(3 * C), yhs=big(C), yhat=big(C)))


def test_dual_prior_host_validation():
    h = K()
    C, H, W = 6, 4, 6
    y, buf, sm, yhat = act(C, H, W), act(4 * C, H, W), act(2 * C, H, W), act(C, H, W)
    buf.buf.fill_(1.0)
    n = (C + 2) // 2 * (H + 1) * (W + 1)
    sym, idx, bits = flat(n, torch.int32), flat(n, torch.int16), flat(n, torch.float32)
    lm, ls = R.NORMAL_TABLE

    def enc(y=y, buf=buf, sm=None, k=0, yhat=yhat):
        h.dp_encode_step(y, buf, sm, k, yhat, None, sym, idx, lm, ls)

    def est(y=y, buf=buf, sm=None, k=0, yhat=yhat):
        h.dp_estimate_step(y, buf, sm, k, yhat, None, bits, 1, 0.11)

    def dec(buf=buf, sm=None, k=0, yhat=yhat):
        h.dp_decode_step(buf, sm, k, sym, yhat, None)

    def ind(buf=buf, sm=None, k=0):
        h.dp_indexes_step(buf, sm, k, idx, lm, ls)

    enc(), est(), dec(), ind(), enc(sm=sm, k=1), est(sm=sm, k=1), dec(sm=sm, k=1), ind(sm=sm, k=1)
    torch.cuda.synchronize()
    taller, wider = (lambda c: act(c, H + 1, W)), (lambda c: act(c, H, W + 1))
    for f in (enc, est, dec, ind):
        invalid(lambda: f(k=-1))
        invalid(lambda: f(k=2, sm=sm))
        invalid(lambda: f(k=0, sm=sm))
        invalid(lambda: f(k=1))
        invalid(lambda: f(buf=act(4 * C + 2, H, W)))          # wrong buf channel count
        invalid(lambda: f(buf=Described(buf, h.BF16)))
        invalid(lambda: f(k=1, sm=act(2 * C + 1, H, W)))
        invalid(lambda: f(k=1, sm=taller(2 * C)))
        invalid(lambda: f(k=1, sm=wider(2 * C)))
        invalid(lambda: f(k=1, sm=Described(sm, h.BF16)))
    # C not a multiple of 2
    y3, b3, o3 = act(3, H, W), act(12, H, W), act(3, H, W)
    invalid(lambda: enc(y=y3, buf=b3, yhat=o3))
    invalid(lambda: est(y=y3, buf=b3, yhat=o3))
    invalid(lambda: dec(buf=b3, yhat=o3))
    invalid(lambda: ind(buf=b3))
    for f in (enc, est, dec):
        for big in (taller, wider):
            invalid(lambda: f(yhat=big(C)))
        invalid(lambda: f(yhat=act(C + 1, H, W)))
    for f in (enc, est):
        for big in (taller, wider):
            invalid(lambda: f(buf=big(4 * C)))
            invalid(lambda: f(buf=big(4 * C), yhat=big(C)))

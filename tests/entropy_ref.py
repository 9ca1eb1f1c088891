"""Plain per-element reference of the entropy-parameter kernels (misc.hip,
hem.hip): the quadtree and dual-prior quantise / index / dequantise steps,
the CDF-index computation and the estimate-mode bit counts.

TEST INFRASTRUCTURE ONLY.  It is a second derivation, independent of the
kernels and of oracle/: where the reference model multiplies whole tensors by
0/1 masks and adds the parts, this file asks, for one (pixel, channel), which
step codes it and with which parameters, and computes that element alone.
Symbols and y_hat are computed in fp32 with numpy (IEEE divide, subtract,
rint = round half to even, add, multiply: each correctly rounded, so there is
one right answer); indexes and bits are evaluated in fp64 from the fp32
inputs.  tests/test_entropy_ref.py pins it against the oracle on the CPU.

Layouts: every map is a (channels, H, W) numpy array.  A step's outputs are
(C/4 or C/2, H, W) arrays whose flattening is the coder order (NCHW of the
tensor the reference hands to the entropy coder).

The second half of the file builds the inputs that both the CPU test and
tests/test_gpu_entropy_kernels.py use.
"""
import math

import numpy as np

F32 = np.float32
SYM_CLAMP = F32(30000.0)      # the int16 coder's symbol range
LN2 = math.log(2.0)

# DCVC-DC forward_four_part_prior names every part y_q_<quarter>_<mask>; read
# off those names, QT_POSITION[k][q] is the mask that channel quarter q uses at
# step k.  mask_m is 1 at 2x2-cell position m = 2 * (row & 1) + (col & 1).
QT_POSITION = ((0, 1, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1), (1, 0, 3, 2))


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def cell_position(H, W):
    """2 * (row & 1) + (col & 1) per pixel.  get_mask_four_parts tiles
    ceil(H/2) x ceil(W/2) cells and crops to H x W, which leaves every kept
    pixel's position in its cell unchanged: odd H and W need nothing more."""
    pos = np.empty((H, W), dtype=np.int64)
    for r in range(H):
        for c in range(W):
            pos[r, c] = 2 * (r % 2) + (c % 2)
    return pos


def quadtree_quarter(k, H, W):
    """(H, W): the channel quarter that step k codes at each pixel."""
    pos = cell_position(H, W)
    quarter = np.empty((H, W), dtype=np.int64)
    for r in range(H):
        for c in range(W):
            quarter[r, c] = QT_POSITION[k].index(int(pos[r, c]))
    return quarter


def dual_half(k, H, W):
    """(H, W): the channel half that step k codes at each pixel.  get_mask's
    mask_0 tiles ((1, 0), (0, 1)): 1 where row + col is even.  Step 0 codes
    half 0 under mask_0 and half 1 under mask_1, step 1 the complement."""
    half = np.empty((H, W), dtype=np.int64)
    for r in range(H):
        for c in range(W):
            even = (r + c) % 2 == 0
            half[r, c] = (0 if even else 1) if k == 0 else (1 if even else 0)
    return half


def gather(x, ch):
    """x[ch[j, r, c], r, c] for a (n, H, W) channel map ch."""
    _, H, W = ch.shape
    return x[ch, np.arange(H)[None, :, None], np.arange(W)[None, None, :]]


def scatter(dst, ch, vals):
    """dst[ch[j, r, c], r, c] = vals[j, r, c]."""
    _, H, W = ch.shape
    dst[ch, np.arange(H)[None, :, None], np.arange(W)[None, None, :]] = vals
    return dst


def _quantise(y_site, qs, mean, sym):
    if sym is None:
        res = y_site / qs - mean          # y / quant_step - means, fp32
        return np.rint(res).astype(F32)   # round half to even
    return np.asarray(sym).reshape(mean.shape).astype(F32)


def quadtree_step(common_params, sm, k, y=None, sym=None):
    """Step k of the quadtree prior for one element per (channel-in-quarter,
    pixel).  common_params = [quant_step | scales | means] (3C channels); sm =
    the spatial prior's [scales | means] (2C) for k > 0, None at k = 0.  With
    ``y`` it is the encoder; with ``sym`` (decoded symbols, coder order) the
    decoder.  Returns a dict of (C/4, H, W) arrays: ch (the channel coded),
    scale, mean, qs (quant_step after the 0.5 clamp), sym_f (fp32 symbol
    before the clamp), sym (after it), yhs (this step's sites of y_hat_so_far)
    and yhat (y_hat * quant_step); and quarter (H, W)."""
    cp = _f32(common_params)
    C = cp.shape[0] // 3
    assert cp.shape[0] == 3 * C and C % 4 == 0 and 0 <= k <= 3 and (sm is None) == (k == 0)
    C4, (H, W) = C // 4, cp.shape[1:]
    quarter = quadtree_quarter(k, H, W)
    ch = quarter[None] * C4 + np.arange(C4)[:, None, None]
    qs = np.maximum(gather(cp, ch), F32(0.5))
    if k == 0:
        scale, mean = gather(cp, C + ch), gather(cp, 2 * C + ch)
    else:
        sm = _f32(sm)
        assert sm.shape == (2 * C, H, W)
        scale, mean = gather(sm, ch), gather(sm, C + ch)
    sym_f = _quantise(None if y is None else gather(_f32(y), ch), qs, mean, sym)
    yhs = sym_f + mean
    return {"quarter": quarter, "ch": ch, "scale": scale, "mean": mean, "qs": qs, "sym_f": sym_f,
            "sym": np.clip(sym_f, -SYM_CLAMP, SYM_CLAMP), "yhs": yhs, "yhat": yhs * qs}


def quadtree_run(common_params, sms, y=None, syms=None):
    """All four steps in order with the spatial prior's outputs given (sms[k-1]
    for step k).  Returns (steps, so_far, yhat): so_far[k] is y_hat_so_far
    after step k (C, H, W), yhat the final y_hat * quant_step."""
    C, (H, W) = common_params.shape[0] // 3, common_params.shape[1:]
    acc, yhat = np.zeros((C, H, W), F32), np.zeros((C, H, W), F32)
    steps, so_far = [], []
    for k in range(4):
        s = quadtree_step(common_params, None if k == 0 else sms[k - 1], k, y=y,
                          sym=None if syms is None else syms[k])
        scatter(acc, s["ch"], s["yhs"])
        scatter(yhat, s["ch"], s["yhat"])
        steps.append(s)
        so_far.append(acc.copy())
    return steps, so_far, yhat


def dual_step(buf, sm, k, y=None, sym=None, post=None):
    """Step k of the dual (checkerboard) prior.  buf = [y_hat_0_0 | y_hat_1_1
    (C) | means (C) | scales (C) | quant_step (C)], the spatial prior's input;
    sm = its output [scales_0 | means_0 | scales_1 | means_1] (C/2 each) for
    k = 1, None at k = 0.  Returns (C/2, H, W) arrays as quadtree_step (symbols
    are int32: sym_f is not clamped), yhat = y_hat * quant_step (* post[ch]),
    half (H, W), and at k = 0 ``buf`` as the step leaves it: section 0 holds
    this step's y_hat at its sites and 0 elsewhere, the quant_step section is
    clamped at 0.5 everywhere, means and scales are untouched."""
    buf = _f32(buf)
    C = buf.shape[0] // 4
    assert buf.shape[0] == 4 * C and C % 2 == 0 and k in (0, 1) and (sm is None) == (k == 0)
    C2, (H, W) = C // 2, buf.shape[1:]
    half = dual_half(k, H, W)
    lane = np.arange(C2)[:, None, None]
    ch, other = half[None] * C2 + lane, (1 - half[None]) * C2 + lane
    qs = np.maximum(gather(buf, 3 * C + ch), F32(0.5))
    if k == 0:
        mean, scale = gather(buf, C + ch), gather(buf, 2 * C + ch)
    else:
        sm = _f32(sm)
        assert sm.shape == (2 * C, H, W)
        scale, mean = gather(sm, half[None] * C + lane), gather(sm, half[None] * C + C2 + lane)
    sym_f = _quantise(None if y is None else gather(_f32(y), ch), qs, mean, sym)
    yh = sym_f + mean
    yhat = yh * qs
    if post is not None:
        yhat = yhat * gather(np.broadcast_to(_f32(post)[:, None, None], (C, H, W)), ch)
    out = {"half": half, "ch": ch, "scale": scale, "mean": mean, "qs": qs, "sym_f": sym_f, "sym": sym_f,
           "yhs": yh, "yhat": yhat}
    if k == 0:
        nb = buf.copy()
        scatter(nb, ch, yh)
        scatter(nb, other, np.zeros_like(yh))
        nb[3 * C:] = np.maximum(buf[3 * C:], F32(0.5))
        out["buf"] = nb
    return out


def dual_run(buf, sm, y=None, syms=None, post=None):
    """Both steps in order.  Returns (steps, buf after step 0, yhat)."""
    C, (H, W) = buf.shape[0] // 4, buf.shape[1:]
    yhat = np.zeros((C, H, W), F32)
    s0 = dual_step(buf, None, 0, y=y, sym=None if syms is None else syms[0], post=post)
    s1 = dual_step(s0["buf"], sm, 1, y=y, sym=None if syms is None else syms[1], post=post)
    for s in (s0, s1):
        scatter(yhat, s["ch"], s["yhat"])
    return [s0, s1], s0["buf"], yhat


# ------------------------------------------------------------------ indexes
def index_float64(scales, log_min, log_step):
    """GaussianEncoder.build_indexes before its clamp and int(): the fp32
    scale, raised to 1e-5 (as fp32 holds it), then evaluated in fp64."""
    s = np.maximum(_f32(scales).astype(np.float64), float(F32(1e-5)))
    return (np.log(s) - log_min) / log_step


def index_of(v):
    """clamp(trunc(v), 0, 255)."""
    return np.clip(np.trunc(v), 0, 255).astype(np.int64)


def near_integer(v, eps):
    return np.abs(v - np.rint(v)) < eps


# --------------------------------------------------------------------- bits
def probs_to_bits(p):
    """-log2(p + 1e-5), not below 0."""
    return np.maximum(-np.log(np.asarray(p, np.float64) + 1e-5) / LN2, 0.0)


def _sigma(sigma, smin):
    # the fp32 clamp sigma.clamp(smin, 1e10): smin as fp32 holds it
    return np.clip(_f32(sigma).astype(np.float64), float(F32(smin)), float(F32(1e10)))


_erf = np.vectorize(math.erf, otypes=[np.float64])


def laplace_prob(yq, sigma, smin):
    """P(yq - 0.5 < X < yq + 0.5), X ~ Laplace(0, clamp(sigma)), in fp64."""
    s, v = _sigma(sigma, smin), _f32(yq).astype(np.float64)

    def cdf(x):
        return 0.5 - 0.5 * np.sign(x) * np.expm1(-np.abs(x) / s)
    return cdf(v + 0.5) - cdf(v - 0.5)


def normal_prob(yq, sigma, smin):
    """P(yq - 0.5 < X < yq + 0.5), X ~ Normal(0, clamp(sigma)), in fp64."""
    s, v = _sigma(sigma, smin), _f32(yq).astype(np.float64)

    def cdf(x):
        return 0.5 * (1.0 + _erf(x / (s * math.sqrt(2.0))))
    return cdf(v + 0.5) - cdf(v - 0.5)


def factorized_prob(z, table):
    """BitEstimator: cdf(z + 0.5) - cdf(z - 0.5) per (channel, pixel) in fp64.
    table[c] = softplus(h1), b1, tanh(a1), ..., softplus(h4), b4 (fp32)."""
    z, t = _f32(z).astype(np.float64), _f32(table).astype(np.float64)
    assert t.shape == (z.shape[0], 11)

    def cdf(x):
        for layer in range(3):
            x = x * t[:, 3 * layer, None, None] + t[:, 3 * layer + 1, None, None]
            x = x + np.tanh(x) * t[:, 3 * layer + 2, None, None]
        x = x * t[:, 9, None, None] + t[:, 10, None, None]
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-x))
    return cdf(z + 0.5) - cdf(z - 0.5)


BITS_FLOOR = 2.0 ** -20   # half an fp32 ulp of the largest bit count (16.6)
ULP = 2.0 ** -24


def bits_K(bits, p):
    """The error of fp32 ``bits`` against probs_to_bits(p) in units of 2^-24
    of probability: max |dbits| (p + 1e-5) ln2 / 2^-24 after the absolute
    floor.  One rounding of a CDF difference near 1 is K = 1."""
    d = np.abs(np.asarray(bits, np.float64).reshape(-1) - probs_to_bits(p).reshape(-1))
    return float((np.maximum(d - BITS_FLOOR, 0.0) * (np.asarray(p).reshape(-1) + 1e-5) * LN2 / ULP).max())


def bits_bound(p, K):
    """Per-element |dbits| allowed at error level K."""
    return K * ULP / ((np.asarray(p, np.float64) + 1e-5) * LN2) + BITS_FLOOR


# =================================================================== inputs
# Shapes (C, H, W): one 2x2 cell; an odd-by-odd map (the mask crop) with a
# quarter that is no power of two; two 256-thread blocks with a partial last
# one.  The dual prior's get_mask is undefined for odd sizes: even only.
QT_SHAPES = ((8, 2, 2), (12, 5, 7), (16, 9, 13))
DP_SHAPES = ((4, 2, 2), (6, 4, 6), (16, 12, 20))
LAPLACE_TABLE = (math.log(0.01), (math.log(64.0) - math.log(0.01)) / 255)   # DCVC-DC scale table
NORMAL_TABLE = (math.log(0.11), (math.log(64.0) - math.log(0.11)) / 255)    # DCVC-HEM scale table
IDX_TIE_EPS = 1e-3      # tests/parity.py
IDX_TIE_SHARE = 0.01    # cap on near-integer indexes among those compared


def _scales(rng, shape, wide):
    """Log-uniform scales ([1e-6, 1e12] when ``wide``, else around the table's
    [0.01, 64]) with engineered ones in fixed slots: 0, negative, below 1e-5,
    above the table's top, 1e12."""
    n = int(np.prod(shape))
    lo, hi = (1e-6, 1e12) if wide else (0.004, 150.0)
    s = np.exp(rng.uniform(math.log(lo), math.log(hi), n))
    slot = (np.arange(n) * 5 + 3) % 11
    s[slot == 5] = 0.0
    s[slot == 6] = -1.5
    s[slot == 7] = 3e-6
    s[slot == 8] = rng.uniform(70.0, 900.0, int((slot == 8).sum()))
    s[slot == 9] = 1e12
    return s.astype(F32).reshape(shape)


def _latent(rng, shape, sources, big, est):
    """y, quant_step and ``sources`` mean maps (one per place a step can read
    its means from).  Engineered elements in fixed slots, with the same mean in
    every source so the element behaves the same whichever step codes it:
    quant_step exactly 0.5 and below it; exact rounding ties (quant_step 1,
    mean a multiple of 0.25, y = mean + n + 0.5); residuals at and beyond the
    +-30000 clamp and up to +-``big``; a zero residual."""
    n = int(np.prod(shape))
    slot = (np.arange(n) * 7 + 1) % 12
    qs = rng.uniform(0.3, 1.3, n)
    y = rng.standard_normal(n) * (12.0 if est else 4.0)
    base = 0.25 * rng.integers(-8, 9, n)
    means = [rng.standard_normal(n) * 1.5 for _ in range(sources)]
    eng = slot >= 7
    for m in means:
        m[eng] = base[eng]
    qs[slot == 5] = 0.5
    qs[slot == 6] = 0.25
    qs[eng] = 1.0
    tie = slot == 7
    y[tie] = base[tie] + rng.integers(-6, 6, int(tie.sum())) + 0.5
    tie2 = slot == 8                      # a tie after a division: quant_step 2
    qs[tie2] = 2.0
    y[tie2] = 2.0 * (base[tie2] + rng.integers(-6, 6, int(tie2.sum())) + 0.5)
    edge = np.array([30001.0, 29999.5, big, 30000.5, 4e4, 30000.4, 32767.6, 32768.5])
    for s, sign in ((9, 1.0), (10, -1.0)):
        m = slot == s
        y[m] = base[m] + sign * edge[np.arange(int(m.sum())) % len(edge)]
    z = slot == 11
    y[z] = base[z] if est else rng.standard_normal(int(z.sum())) * 300.0
    f = lambda a: a.astype(F32).reshape(shape)  # noqa: E731
    return f(y), f(qs), [f(m) for m in means]


def quadtree_case(C, H, W, est=False):
    """Inputs of the four quadtree steps: y (C), params = [quant_step | scales
    | means] (3C) and the three spatial-prior outputs sms[k-1] = [scales |
    means] (2C).  ``est``: sigma log-uniform over [1e-6, 1e12] and wider
    symbols, for the estimate-mode bits."""
    rng = np.random.default_rng(1000 * C + 10 * H + W + (500000 if est else 0))
    y, qs, means = _latent(rng, (C, H, W), 4, 1e5, est)
    scales = [_scales(rng, (C, H, W), est) for _ in range(4)]
    return {"y": y, "params": np.concatenate([qs, scales[0], means[0]]),
            "sms": [np.concatenate([scales[k], means[k]]) for k in (1, 2, 3)]}


def dual_case(C, H, W, est=False):
    """Inputs of the two dual-prior steps: y (C), buf (4C, section 0 is
    overwritten by step 0), sm = [scales_0 | means_0 | scales_1 | means_1] and
    a per-channel post_scale."""
    rng = np.random.default_rng(77000 + 1000 * C + 10 * H + W + (500000 if est else 0))
    y, qs, means = _latent(rng, (C, H, W), 2, 1e6, est)
    scales = [_scales(rng, (C, H, W), est) for _ in range(2)]
    C2 = C // 2
    buf = np.concatenate([np.full((C, H, W), 7.25, F32), means[0], scales[0], qs])
    sm = np.concatenate([scales[1][:C2], means[1][:C2], scales[1][C2:], means[1][C2:]])
    return {"y": y, "buf": buf, "sm": sm, "post": rng.uniform(0.5, 2.0, C).astype(F32)}


def bits_grid():
    """Integer y_q in [-40, 40] against sigma log-uniform over [1e-6, 1e12]."""
    rng = np.random.default_rng(4242)
    n = 4096
    return (rng.integers(-40, 41, n).astype(F32),
            np.exp(rng.uniform(math.log(1e-6), math.log(1e12), n)).astype(F32))


def estimate_pairs(kind):
    """Every (y_q, sigma) pair that the GPU estimate tests feed the kernels
    (kind "quadtree" or "dual"), followed by bits_grid()."""
    yq, sg = [], []
    if kind == "quadtree":
        for shape in QT_SHAPES:
            c = quadtree_case(*shape, est=True)
            for s in quadtree_run(c["params"], c["sms"], y=c["y"])[0]:
                yq.append(s["sym_f"].reshape(-1))
                sg.append(s["scale"].reshape(-1))
    else:
        for shape in DP_SHAPES:
            c = dual_case(*shape, est=True)
            for s in dual_run(c["buf"], c["sm"], y=c["y"])[0]:
                yq.append(s["sym_f"].reshape(-1))
                sg.append(s["scale"].reshape(-1))
    g = bits_grid()
    return np.concatenate(yq + [g[0]]), np.concatenate(sg + [g[1]])


FACTORIZED_SHAPES = ((3, 5, 7), (5, 9, 13))


def factorized_case(C, H, W):
    """A BitEstimator's raw parameters (h, b, a of 4 Bitparm layers; a of the
    first three), the [C][11] table the kernel reads (softplus(h), b, tanh(a)
    in fp32 with torch's own ops, as dcvc_amd.entropy builds it) and integer z
    in [-40, 40] (C, H, W)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(31000 + 100 * C + H)
    raw, cols = {}, []
    for i in range(1, 5):
        h = torch.from_numpy((rng.standard_normal(C) * 0.5 + 0.3).astype(F32))
        b = torch.from_numpy((rng.standard_normal(C) * 0.5).astype(F32))
        raw[f"f{i}.h"], raw[f"f{i}.b"] = h, b
        cols += [F.softplus(h), b]
        if i < 4:
            a = torch.from_numpy((rng.standard_normal(C) * 0.5).astype(F32))
            raw[f"f{i}.a"] = a
            cols.append(torch.tanh(a))
    table = torch.stack(cols, dim=1).contiguous().numpy()
    z = rng.integers(-40, 41, (C, H, W)).astype(F32)
    return {"raw": raw, "table": table, "z": z}

"""dcvc_digest (digest.hip) against a numpy implementation of its definition
(INTEGRATION.md "DPB digest"), written here from the text.  Equality is exact:
the digest is integer arithmetic."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
PHI = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def K():
    from dcvc_amd import hip
    return hip


def ref_digest(view, seed):
    """view: numpy (H, W, C) of uint32 (fp32 bit patterns) or uint16 (bf16 bit
    patterns), the logical view whatever buffer it was cut from."""
    bits = np.ascontiguousarray(view).reshape(-1)
    neg_zero = 0x80000000 if bits.dtype == np.uint32 else 0x8000
    b = np.where(bits == neg_zero, 0, bits).astype(np.uint64)
    n = np.arange(b.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = ((b << np.uint64(32)) | n) + np.uint64((seed * PHI) & M64)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return int(np.add.reduce(z)) & M64, int(np.bitwise_xor.reduce(z))


def bits_of(t):
    """torch (H, W, C) fp32 / bf16 tensor (any strides) -> numpy bit patterns."""
    t = t.contiguous().cpu()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def gpu_digest(act, seed, out=None):
    h = K()
    if out is None:
        out = torch.zeros(2, dtype=torch.int64, device=act.buf.device)
    h.digest(act, seed, out)
    return tuple(int(v) & M64 for v in out.cpu().tolist())


def rand_act(H, W, C, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(H, W, C, generator=g) * 3).to(dtype)
    return K().Act(t.cuda())


# name -> (H, W, Cbuf, window or None, dtype)
CASES = {
    "1x1x1": (1, 1, 1, None, torch.float32),
    "3x5x3 scalar, odd": (3, 5, 3, None, torch.float32),
    "17x33x4 vector": (17, 33, 4, None, torch.float32),
    "window ch(5,13) of 2x7x48": (2, 7, 48, (5, 13), torch.float32),
    "window ch(16,32) of 64, vector": (5, 9, 64, (16, 32), torch.float32),
    "9x11x6 bf16": (9, 11, 6, None, torch.bfloat16),
    "6x10x16 bf16 vector": (6, 10, 16, None, torch.bfloat16),
    "window ch(8,8) of 24 bf16 vector": (4, 5, 24, (8, 8), torch.bfloat16),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_digest_matches_definition(name):
    H, W, C, win, dtype = CASES[name]
    a = rand_act(H, W, C, dtype, seed=len(name))
    v = a if win is None else a.ch(*win)
    for seed in (1, 5, M64):
        ref = ref_digest(bits_of(v.t()), seed)
        assert gpu_digest(v, seed) == ref, (name, seed)
        if win is not None:
            # pitch and channel offset do not enter: a contiguous copy digests the same
            assert gpu_digest(K().Act(v.t().contiguous()), seed) == ref, (name, seed)


def test_grid_stride_passes():
    """A shape at which every thread of the full grid runs its loop more than
    twice and the last pass is partial, on both paths.  The geometry is the
    kernel's (dcvc_digest_threads(): T threads, 4 blocks of 256 per CU): a
    pass of the 16-byte path covers 2 T items of 4 fp32 channels, a pass of
    the scalar path T elements; 5.5 T items / elements give two full passes
    and a third one that half the threads (16-byte path: half of their second
    load) take.  On an MI355X, T = 262144 and the shapes are 1408 x 512 x 8
    (vector) and 704 x 512 x 4 with a one-channel-wider pitch (scalar)."""
    h = K()
    T = h.digest_threads()
    W = 512
    assert (11 * T) % (8 * W) == 0
    # (C, pitch, items per pixel, items per pass)
    for C, pitch, per_pix, per_pass in ((8, 8, 2, 2 * T), (4, 5, 4, T)):
        H = 11 * T // (2 * per_pix * W)          # H * W * per_pix = 5.5 T
        a = rand_act(H, W, pitch, seed=C)
        v = a if pitch == C else a.ch(1, C)
        work = H * W * per_pix
        assert 2 * work == 11 * T and work > 2 * per_pass and work % per_pass != 0
        assert gpu_digest(v, 3) == ref_digest(bits_of(v.t()), 3), C


def test_order_matters():
    a = rand_act(7, 9, 5, seed=3)
    t = a.buf
    assert t[0, 0, 0] != t[6, 8, 4]
    d0 = gpu_digest(a, 1)
    t[0, 0, 0], t[6, 8, 4] = t[6, 8, 4].clone(), t[0, 0, 0].clone()
    d1 = gpu_digest(a, 1)
    assert d0 != d1 and d0[0] != d1[0] and d0[1] != d1[1]
    assert d1 == ref_digest(bits_of(t), 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_signs_are_one_value(dtype):
    a = rand_act(4, 6, 8, dtype, seed=4)
    a.buf[1, 2, 3] = 0.0
    a.buf[3, 5, 7] = -0.0
    d0 = gpu_digest(a, 2)
    a.buf[1, 2, 3] = -0.0
    a.buf[3, 5, 7] = 0.0
    assert bool(torch.signbit(a.buf[1, 2, 3])) and not bool(torch.signbit(a.buf[3, 5, 7]))
    assert gpu_digest(a, 2) == d0 == ref_digest(bits_of(a.buf), 2)


def test_nan_payloads_count():
    a = rand_act(3, 4, 4, seed=5)
    iv = a.buf.view(torch.int32)
    iv[1, 1, 1] = 0x7FC00000
    d0 = gpu_digest(a, 1)
    iv[1, 1, 1] = 0x7FC00001
    d1 = gpu_digest(a, 1)
    assert d0 != d1
    assert d1 == ref_digest(bits_of(a.buf), 1)


def test_fold_and_repeat():
    """Two calls into one out equal the host-side fold (add, xor) of the two
    separate results; the same call twice gives the same words."""
    a, b = rand_act(5, 7, 12, seed=6), rand_act(3, 3, 2, torch.bfloat16, seed=7)
    da, db = gpu_digest(a, 1), gpu_digest(b, 2)
    assert gpu_digest(a, 1) == da and gpu_digest(b, 2) == db
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    gpu_digest(a, 1, out)
    both = gpu_digest(b, 2, out)
    assert both == ((da[0] + db[0]) & M64, da[1] ^ db[1])
    assert da != gpu_digest(a, 2)

"""tests/hygiene.py itself: the embedding on the CPU, and three GPU self-tests
showing that the net catches a view that is declared larger than its data.

The self-tests use dcvc_copy only, and every access stays inside the
allocation: a widened view reaches one channel or one row into its own guard
band.  Each runs the check once with the deliberate view error, which must
raise HygieneError, and once without it, which must pass.
"""
import pytest
import torch

from dcvc_amd import hip as K
from tests import hygiene as HY

gpu = pytest.mark.gpu
CPU = torch.device("cpu")
C, H, W = 16, 5, 7


def data(c=C, h=H, w=W, seed=0):
    return torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(seed))


# --------------------------------------------------------------------- CPU
@pytest.mark.parametrize("dtype", [K.F32, K.BF16])
@pytest.mark.parametrize("fill", HY.FILLS)
@pytest.mark.parametrize("lead", [8, 2])
def test_embed_layout(dtype, fill, lead):
    x = data()
    a = HY.embed(x, dtype, lead=lead, fill=fill, device=CPU)
    tdt = torch.float32 if dtype == K.F32 else torch.bfloat16
    assert (a.H, a.W, a.C, a.coff) == (H, W, C, lead)
    assert a.big.shape == (HY.ROWS + H + HY.ROWS, W, lead + C + HY.TAIL) and a.buf.is_contiguous()
    assert a.buf.data_ptr() == a.big.data_ptr() + HY.ROWS * W * a.big.shape[2] * a.big.element_size()
    assert a.buf.data_ptr() % 16 == 0
    assert torch.equal(a.nchw(), x.to(tdt).float())
    # everything outside the view holds the fill
    out = torch.ones(a.big.shape, dtype=torch.bool)
    out[HY.ROWS:HY.ROWS + H, :, lead:lead + C] = False
    v = a.big[out]
    if fill == "zero":
        assert not v.any()
    elif fill == "nan":
        assert bool(torch.isnan(v).all())
        assert bool((v.view(torch.int32 if dtype == K.F32 else torch.int16) == -1).all())
    else:
        assert bool((v.float() >= 2.0 ** 15).all()) and bool(torch.isfinite(v).all())
        assert bool(torch.isinf(v.float().half()).all())      # Inf after an fp16 split
    assert HY.guards_intact(a) and HY.fully_written(a)


def test_output_view_and_guards():
    y = HY.embed_out(C, H, W, K.F32, device=CPU)
    assert bool(torch.isnan(y.t()).all()) and not HY.fully_written(y)
    assert bool((y.big.view(torch.uint8)[:HY.ROWS] == HY.CANARY_BYTE).all())
    y.t().copy_(data()[0].permute(1, 2, 0))
    assert HY.fully_written(y) and HY.guards_intact(y)
    y.t()[2, 3, 4] = float("nan")
    assert not HY.fully_written(y)
    with pytest.raises(HY.HygieneError, match="1 elements of the view hold NaN"):
        HY.check_written(y, "y")
    # one element in each guard band: a channel before, a channel after, a row above, a row below
    for idx in ((HY.ROWS, 0, HY.LEAD - 1), (HY.ROWS, 0, HY.LEAD + C), (HY.ROWS - 1, 0, HY.LEAD),
                (HY.ROWS + H, W - 1, HY.LEAD + C - 1)):
        y = HY.embed_out(C, H, W, K.BF16, device=CPU)
        assert HY.guards_intact(y)
        y.big[idx] = 1.0
        assert not HY.guards_intact(y) and HY.outside_changes(y) == 2
        with pytest.raises(HY.HygieneError, match="outside the view"):
            HY.check_guards(y, "y")
    # a store of the very value the guard holds is the one thing a byte compare cannot see
    y = HY.embed_out(C, H, W, K.F32, device=CPU)
    y.big[0, 0, 0] = y.big[0, 0, 1]
    assert HY.guards_intact(y)


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.uint8, torch.float32, torch.float64])
def test_raw_arguments(dtype):
    n = 37
    d = torch.arange(n).to(dtype)
    for fill in HY.FILLS:
        v = HY.embed_raw(d, fill, device=CPU)
        big = v._hyg[0]
        assert v.numel() == n and v.is_contiguous() and torch.equal(v, d) and big.numel() == n + 2 * HY.GUARD
        assert (v.data_ptr() - big.data_ptr()) % 16 == 0
        g = torch.cat([big[:HY.GUARD], big[HY.GUARD + n:]])
        if fill == "zero":
            assert not g.any()
        elif dtype.is_floating_point:
            assert bool(torch.isnan(g).all()) if fill == "nan" else bool((g == HY.BIG).all())
        else:
            info = torch.iinfo(dtype)
            assert bool((g == (info.min if fill == "nan" else info.max)).all())
        assert HY.guards_intact(v)
        big[HY.GUARD - 1] = 1
        assert not HY.guards_intact(v)
    o = HY.embed_raw_out(n, dtype, device=CPU)
    assert HY.guards_intact(o) and HY.fully_written(o) != dtype.is_floating_point
    o._hyg[0][HY.GUARD + n] = 3
    assert not HY.guards_intact(o)


def test_same_bits_and_refs():
    a = {"y": torch.tensor([1, 2, 3])}
    HY.check_same_bits(a, {"y": torch.tensor([1, 2, 3])})
    with pytest.raises(HY.HygieneError, match="differs from the clean run in 1 elements"):
        HY.check_same_bits(a, {"y": torch.tensor([1, 2, 4])}, "t")
    env = HY.Env("zero", {}, device=CPU, dry=True)
    y = env.y("y", C, H, W)
    y.t().copy_(data()[0].permute(1, 2, 0))
    env.ref("y", lambda: data().double(), None)
    HY.check_refs(env, "t")
    env.ref("y", lambda: data().double() * (1 + 1e-5), 1e-6)
    with pytest.raises(HY.HygieneError, match="rel error"):
        HY.check_refs(env, "t")


# -------------------------------------------------- GPU: the net catches something
def copy_entry(src_wider=0, src_taller=0, dst_wider=0):
    """dcvc_copy of a C-channel, H-row tensor between two embedded views.
    src_wider / src_taller declare the SOURCE view one channel / one row larger
    than the data (the surplus lies in the source's own guard band; the
    destination is made as large, so the copy itself is well formed).
    dst_wider hands the kernel a DESTINATION one channel wider than the view
    the test guards (the source carries real data for it)."""
    def fn(E):
        x = E.randn("x", 1, C + dst_wider, H, W)
        xa = E.x(x)
        y = E.y("y", C + src_wider, H + src_taller, W)
        src = K.Act(xa.big[xa.rows:xa.rows + H + src_taller], xa.lead, C + src_wider + dst_wider)
        dst = K.Act(y.buf, y.lead, y.C + dst_wider)
        E.launch(K.copy, src, dst)
    return fn


def expect_caught(fn, match):
    with pytest.raises(HY.HygieneError, match=match) as e:
        HY.run_entry(fn, "copy self-test", fills=("big", "nan"))
    print("caught as designed:", e.value)


@pytest.fixture
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@gpu
def test_net_passes_a_well_formed_copy(_gpu):
    HY.run_entry(copy_entry(), "copy self-test")


@gpu
def test_net_catches_source_one_channel_wider(_gpu):
    expect_caught(copy_entry(src_wider=1), r"\[big\]: output 'y' differs from the clean run in 35 elements")


@gpu
def test_net_catches_source_one_row_taller(_gpu):
    expect_caught(copy_entry(src_taller=1), rf"\[big\]: output 'y' differs from the clean run in {W * C} elements")


@gpu
def test_net_catches_destination_one_channel_wider(_gpu):
    expect_caught(copy_entry(dst_wider=1), r"output 'y': \d+ bytes outside the view were written")

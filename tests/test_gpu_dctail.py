"""sdct.hip: the tail of a feature-rate DepthConv in one kernel,
  out = conv2(dw3x3(t) + bdw) + b2 + (adaptor(x) + ba | x),
bit-identical to the launches it replaces (K.dwconv3x3, K.conv(adaptor),
K.conv(conv2, res=idn)) for every instantiation.

Map sizes: the kernel walks 8 x 16 pixel tiles with one persistent workgroup
per CU, so 1x1 is a single pixel, 3x5 a map smaller than a tile, 8x16 exactly
one tile, 9x17 one past a tile in both directions, 23x37 several ragged tiles,
and 130x270 (17 x 17 = 289 tiles) more tiles than a 256-CU device has
workgroups: the only size at which a workgroup carries its load pipeline from
one tile into the next.
"""
import pytest
import torch

from tests import hygiene as HY

gpu = pytest.mark.gpu

# (c = cx, cout, adaptor) of the instantiations
INST = [(128, 64, True), (64, 128, True), (128, 128, False)]
SIZES = [(1, 1), (3, 5), (8, 16), (9, 17), (23, 37), (130, 270)]


def K():
    from dcvc_amd import hip
    return hip


class Block:
    """Seeded weights of one DepthConv tail, packed for both routes."""

    def __init__(self, c, cout, adapt, center_only=False):
        h = K()
        g = torch.Generator().manual_seed(c * 1000 + cout * 2 + adapt)
        self.c, self.cout, self.adapt = c, cout, adapt
        wd = torch.randn(c, 1, 3, 3, generator=g) / 3
        bd = torch.randn(c, generator=g) * 0.1
        if center_only:   # the depthwise conv as the identity: its output is t, exactly
            wd = torch.zeros(c, 1, 3, 3)
            wd[:, 0, 1, 1] = 1.0
            bd = torch.zeros(c)
        w2 = torch.randn(cout, c, 1, 1, generator=g) / c ** 0.5
        b2 = torch.randn(cout, generator=g) * 0.1
        wa = torch.randn(cout, c, 1, 1, generator=g) / c ** 0.5 if adapt else None
        ba = torch.randn(cout, generator=g) * 0.1 if adapt else None
        self.w9c = wd.reshape(c, 9).t().contiguous().cuda()
        self.bd = bd.cuda()
        self.c2 = h.ConvW(w2, b2, 1, h.F16X3)
        self.ca = h.ConvW(wa, ba, 1, h.F16X3) if adapt else None
        self.tw = h.DcTailW(self.w9c, self.bd, w2, b2, wa, ba)
        self.dwc = h.DwcW(self.w9c, self.bd, w2, b2) if not adapt else None

    def unfused(self, t, x, y=None):
        h = K()
        d = h.dwconv3x3(t, self.w9c, self.bd)
        idn = h.conv(self.ca, x) if self.adapt else x
        return h.conv(self.c2, d, y, res=idn)

    def fused(self, t, x, y=None):
        h = K()
        out = h.dc_tail_split(self.tw, t, x, y)
        if out is not None:
            assert h.lib().dcvc_last_kernel().decode().startswith("sdct_kernel"), h.lib().dcvc_last_kernel()
        return out

    def routed(self, t, x, y=None):
        """As DepthConvBlock routes it: the kernel, else the earlier route."""
        out = K().dc_tail_split(self.tw, t, x, y)
        return out if out is not None else self.unfused(t, x, y)


_BLOCKS = {}


def block(c, cout, adapt):
    if (c, cout, adapt) not in _BLOCKS:
        _BLOCKS[(c, cout, adapt)] = Block(c, cout, adapt)
    return _BLOCKS[(c, cout, adapt)]


def inputs(c, H, W, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + c * 31 + H * 1000 + W)
    return torch.randn(1, c, H, W, generator=g), torch.randn(1, c, H, W, generator=g)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@gpu
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("c,cout,adapt", INST)
def test_tail_is_bit_identical_to_the_unfused_route(c, cout, adapt, H, W):
    need_gpu()
    h = K()
    B = block(c, cout, adapt)
    t, x = inputs(c, H, W)
    ta, xa = h.from_nchw(t), h.from_nchw(x)
    want = B.unfused(ta, xa)
    got = B.fused(ta, xa)
    assert got is not None
    torch.cuda.synchronize()
    assert torch.equal(got.buf, want.buf)
    if not adapt:
        # the latent-rate kernel the 128-channel blocks ran before
        old = h.dw_conv2_split(B.dwc, ta, xa)
        assert old is not None and h.lib().dcvc_last_kernel().decode().startswith("sldc_kernel")
        torch.cuda.synchronize()
        assert torch.equal(got.buf, old.buf)


@gpu
@pytest.mark.parametrize("H,W", [(9, 17), (23, 37)])
def test_tail_on_channel_views_ignores_their_surroundings(H, W):
    """x = channels [64, 192) of a 192-channel buffer, y = channels [0, 64) of
    a 128-channel one (the UNet's concat buffers), t inside a wider buffer
    too, each with guard rows above and below: NaN or 1e30 around the views
    changes no output bit, nothing outside y's window is written, every
    element of it is, and LDS / VGPR poison before the launch changes nothing."""
    need_gpu()
    B = block(128, 64, True)
    t, x = inputs(128, H, W, seed=1)
    runs = {}
    for fill, poison in (("zero", False), ("nan", False), ("big", False), ("zero", True)):
        ta = HY.embed(t, fill=fill)
        xa = HY.embed(x, lead=64, tail=0, fill=fill)
        ya = HY.embed_out(64, H, W, lead=0, tail=64)
        assert xa.buf.shape[2] == 192 and xa.coff == 64 and ya.buf.shape[2] == 128 and ya.coff == 0
        if poison:
            HY.poison_on_stream()
        assert B.fused(ta, xa, ya) is not None
        torch.cuda.synchronize()
        HY.check_guards(ya, f"y ({fill})")
        HY.check_written(ya, f"y ({fill})")
        for a in (ta, xa):
            HY.check_guards(a, f"input ({fill})")
        runs[(fill, poison)] = HY.bits_of(ya)
    first = runs[("zero", False)]
    for k, v in runs.items():
        assert torch.equal(v, first), k
    want = B.unfused(K().from_nchw(t), K().from_nchw(x))
    torch.cuda.synchronize()
    assert torch.equal(HY.bits_of(want), first)


@gpu
def test_misaligned_view_takes_the_fallback():
    """x at channel offset 2 (no 16-byte pieces): DCVC_HIP_EUNSUPPORTED, and
    the earlier route gives what the kernel gives for the same values."""
    need_gpu()
    h = K()
    B = block(128, 64, True)
    t, x = inputs(128, 9, 17, seed=2)
    ta = h.from_nchw(t)
    xa = HY.embed(x, lead=2, tail=2, rows=0)
    assert h.dc_tail_split(B.tw, ta, xa) is None
    got = B.routed(ta, xa)
    want = B.fused(ta, h.from_nchw(x))
    torch.cuda.synchronize()
    assert torch.equal(got.buf, want.buf)


@gpu
def test_too_large_map_takes_the_fallback():
    """x as a 128-channel window of a buffer past the 0x7fff0000-byte bound
    of a 32-bit buffer offset (256 x 256 pixels, 8320 channels apart):
    DCVC_HIP_EUNSUPPORTED from the kernel and from sldc_kernel, and the
    unfused route gives what the kernel gives for the same values."""
    need_gpu()
    h = K()
    B = block(128, 128, False)
    H = W = 256
    g = torch.Generator(device="cuda").manual_seed(5)
    wide = torch.empty((H, W, 8320), dtype=torch.float32, device="cuda")
    assert wide.numel() * 4 > 0x7fff0000
    wide[:, :, :128] = torch.randn((H, W, 128), generator=g, device="cuda")
    xa = h.Act(wide, 0, 128)
    ta = h.Act(torch.randn((H, W, 128), generator=g, device="cuda"))
    assert h.dc_tail_split(B.tw, ta, xa) is None
    assert h.dw_conv2_split(B.dwc, ta, xa) is None
    got = B.routed(ta, xa)
    want = B.fused(ta, h.Act(wide[:, :, :128].contiguous()))
    torch.cuda.synchronize()
    assert torch.equal(got.buf, want.buf)


@gpu
@pytest.mark.parametrize("c,cout,adapt", INST)
def test_range_guard_trips_exactly_when_the_unfused_route_does(c, cout, adapt):
    """The depthwise output enters conv2's split: at 2^15 the flag is raised,
    one ulp below it is not, as in the unfused route (whose conv2 launch
    splits the same values); an in-range launch afterwards leaves it clear.
    The depthwise conv is the identity here, so its output is t exactly."""
    need_gpu()
    h = K()
    B = Block(c, cout, adapt, center_only=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    below = float(torch.nextafter(torch.tensor(32768.0), torch.tensor(0.0)))
    try:
        for peak, want in ((32768.0, True), (-32768.0, True), (below, False), (1.0, False)):
            t, x = inputs(c, 9, 17, seed=3)
            t[0, c - 1, 8, 16] = peak          # the last pixel of the ragged second tile row
            ta, xa = h.from_nchw(t), h.from_nchw(x)
            trips = []
            for run in (B.unfused, B.fused):
                h.split_guard_arm(dev)
                assert run(ta, xa) is not None
                trips.append(h.split_guard_tripped())
            assert trips == [want, want], (peak, trips)
    finally:
        h.split_guard_disarm()


@gpu
@pytest.mark.parametrize("H,W", [(9, 17), (23, 37)])
@pytest.mark.parametrize("c,cout,adapt", INST)
def test_tail_is_repeatable(c, cout, adapt, H, W):
    """20 launches on one stream into the same output: identical bits (the
    tile and chunk buffers carry nothing from one launch into the next)."""
    need_gpu()
    h = K()
    B = block(c, cout, adapt)
    t, x = inputs(c, H, W, seed=4)
    ta, xa = h.from_nchw(t), h.from_nchw(x)
    y = h.empty(H, W, cout, h.F32)
    outs = []
    for _ in range(20):
        assert B.fused(ta, xa, y) is not None
        outs.append(y.buf.view(torch.int32).clone())   # (a copy on the same stream)
    torch.cuda.synchronize()
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


@gpu
def test_option_routes_the_tail_back():
    """dctail = 0: DCVC_HIP_EUNSUPPORTED for every shape, same results."""
    need_gpu()
    h = K()
    B = block(64, 128, True)
    t, x = inputs(64, 9, 17, seed=6)
    ta, xa = h.from_nchw(t), h.from_nchw(x)
    want = B.fused(ta, xa)
    assert h.get_option("dctail") == 1
    h.set_option("dctail", 0)
    try:
        assert h.dc_tail_split(B.tw, ta, xa) is None
        got = B.routed(ta, xa)
    finally:
        h.set_option("dctail", 1)
    torch.cuda.synchronize()
    assert torch.equal(got.buf, want.buf)


def test_option_is_registered_and_on():
    h = K()
    assert h.get_option("dctail") == 1

"""The host side of GOP lanes (dcvc_amd/lanes.py and what it needs from the
readers and the sequence file), without a GPU: GOP ranges, the header-walk
index of a sequence file, random access to every source reader, and the lane
pool's ordering, memory bound and failure handling on lanes that compute
nothing.
"""
import struct
import threading

import numpy as np
import pytest

from dcvc_amd import lanes as L
from dcvc_amd.sequence import (FLAG_DIGEST, FLAG_TWIN, SequenceFormatError, SequenceReader, SequenceWriter)


# ------------------------------------------------------------------ ranges
@pytest.mark.parametrize("n, gop, want", [
    (11, 4, [(0, 4), (4, 8), (8, 11)]),
    (8, 8, [(0, 8)]),
    (1, 32, [(0, 1)]),
    (9, 8, [(0, 8), (8, 9)]),
])
def test_gop_ranges(n, gop, want):
    assert L.gop_ranges(n, gop) == want


def test_gop_ranges_edges():
    assert L.gop_ranges(0, 4) == []
    with pytest.raises(ValueError):
        L.gop_ranges(4, 0)


# ------------------------------------------------------------------- index
# (type, payload, twin, digest): irregular I positions, an empty payload, both flags
RECORDS = [("I", b"abc", False, (1, 2)), ("P", b"", False, None), ("P", b"x" * 300, True, (3, 4)),
           ("I", b"\x00\x01", True, None), ("I", b"q" * 7, False, (2 ** 64 - 1, 5)), ("P", b"zz", False, (6, 7)),
           ("P", b"y", False, (8, 9))]


@pytest.fixture()
def seq_file(tmp_path):
    path = str(tmp_path / "made_up.seq")
    with SequenceWriter(path, "DC", "rgb", "split", 130, 100) as wr:
        for t, payload, twin, digest in RECORDS:
            wr.write(t, payload, twin=twin, digest=digest)
    return path


def test_index_matches_the_bytes(seq_file):
    raw = open(seq_file, "rb").read()
    with SequenceReader(seq_file) as r:
        index = r.index()
        records = list(r)                     # the sequential cursor was left at the first record
    assert len(index) == len(records) == len(RECORDS)
    for i, (e, rec, (t, payload, twin, digest)) in enumerate(zip(index, records, RECORDS)):
        assert (e.frame_idx, e.type, e.length) == (i, t, len(payload))
        assert e.flags == (FLAG_TWIN if twin else 0) | (FLAG_DIGEST if digest is not None else 0)
        assert raw[e.offset:e.offset + e.length] == payload == rec["payload"]
        ftype, flags, _, n, s, x = struct.unpack("<BBHIQQ", raw[e.offset - 24:e.offset])
        assert ("IP"[ftype], flags, n) == (t, e.flags, e.length)
        assert ((s, x) if digest is not None else None) == digest == rec["digest"]
    assert index[-1].offset + index[-1].length == len(raw)
    assert L.gops_of(index) == [(0, 3), (3, 4), (4, 7)]


def test_index_reads_no_payload(seq_file):
    """The walk reads the 24-byte headers only."""
    with SequenceReader(seq_file) as r:
        inner, seen = r.file, []

        class Spy:
            def read(self, n=-1):
                seen.append(n)
                return inner.read(n)

            def __getattr__(self, name):
                return getattr(inner, name)
        r.file = Spy()
        r.index()
        r.file = inner
    assert seen == [24] * len(RECORDS)


def test_records_from(seq_file):
    with SequenceReader(seq_file) as r:
        index, everything = r.index(), list(r)
        assert list(r.records_from(index[3])) == everything[3:]
        assert list(r.records_from(index[4], 2)) == everything[4:6]
        assert list(r.records_from(index[0], 3)) == everything[:3]
        assert list(r.records_from(index[6], 5)) == everything[6:]


def test_index_of_damaged_files(seq_file, tmp_path):
    raw = open(seq_file, "rb").read()
    for cut in (1, 2 + 24, 2 + 24 + 1 + 24 - 5):      # in the last payload, in its header, in the header before
        bad = str(tmp_path / f"cut{cut}.seq")
        with open(bad, "wb") as f:
            f.write(raw[:len(raw) - cut])
        with SequenceReader(bad) as r, pytest.raises(SequenceFormatError, match="truncated"):
            r.index()
    unclosed = str(tmp_path / "unclosed.seq")
    wr = SequenceWriter(unclosed, "DC", "rgb", "split", 130, 100)
    wr.write("I", b"abc")
    wr.file.flush()
    with pytest.raises(SequenceFormatError, match="not closed"):
        SequenceReader(unclosed).index()
    wr.close()
    with SequenceReader(unclosed) as r:
        assert [e.type for e in r.index()] == ["I"]
    with open(str(tmp_path / "p_first.seq"), "wb") as f:
        f.write(raw)
    with SequenceWriter(str(tmp_path / "p_first.seq"), "DC", "rgb", "split", 130, 100) as wr:
        wr.write("P", b"abc")
    with SequenceReader(str(tmp_path / "p_first.seq")) as r, pytest.raises(SequenceFormatError, match="P frame"):
        L.gops_of(r.index())


# ----------------------------------------------------------- random access
H, W, N = 6, 8, 5


def _same(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _check_random_access(make, dst_format):
    """read_frame(i) is the i-th sequential read, past the end included, in any
    order, and leaves a sequential reader's cursor alone."""
    seq = make()
    want = [seq.read_one_frame(dst_format) for _ in range(N + 2)]
    assert not _same(want[N - 1], want[N]) and _same(want[N], want[N + 1])     # N frames, then the end
    rnd = make()
    for i in (3, 0, N + 1, N - 1, N, 1, 2, 3):
        assert _same(rnd.read_frame(i, dst_format), want[i]), i
    both = make()
    for i in range(N + 1):
        assert _same(both.read_frame((i * 3) % N, dst_format), want[(i * 3) % N])
        assert _same(both.read_one_frame(dst_format), want[i]), i
    with pytest.raises(ValueError):
        rnd.read_frame(-1, dst_format)
    for r in (seq, rnd, both):
        r.close()


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("fmt", ["420", "422", "444"])
def test_yuv_read_frame(fmt, depth, tmp_path):
    from dcvc_amd.harness import YUVReader
    rng = np.random.default_rng(1)
    sx, sy = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[fmt]
    per = H * W + 2 * (H // sy) * (W // sx)
    dtype = np.uint8 if depth == 8 else "<u2"
    data = rng.integers(0, 1 << depth, size=N * per + 3).astype(dtype)      # 3 samples of a cut-short frame
    path = str(tmp_path / "src.yuv")
    data.tofile(path)
    _check_random_access(lambda: YUVReader(path, W, H, src_format=fmt, bit_depth=depth), "420")
    skipped = YUVReader(path, W, H, src_format=fmt, skip_frame=2, bit_depth=depth)
    assert _same(skipped.read_frame(1), YUVReader(path, W, H, src_format=fmt, bit_depth=depth).read_frame(3))
    assert _same(skipped.read_frame(N - 2), (None, None))


@pytest.mark.parametrize("depth", [8, 10])
def test_rgb_read_frame(depth, tmp_path):
    from dcvc_amd.harness import RGBReader
    rng = np.random.default_rng(2)
    data = rng.integers(0, 1 << depth, size=N * 3 * H * W + 5).astype(np.uint8 if depth == 8 else "<u2")
    path = str(tmp_path / "src.rgb")
    data.tofile(path)
    _check_random_access(lambda: RGBReader(path, W, H, bit_depth=depth), "rgb")


@pytest.mark.parametrize("pad", [1, 5])
def test_png_read_frame(pad, tmp_path):
    from PIL import Image
    from dcvc_amd.harness import PNGReader
    rng = np.random.default_rng(3)
    for t in range(N):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(
            str(tmp_path / f"im{str(t + 1).zfill(pad)}.png"))
    _check_random_access(lambda: PNGReader(str(tmp_path), W, H), "rgb")


@pytest.mark.parametrize("dst", ["rgb", "420"])
def test_array_read_frame(dst):
    from dcvc_amd.harness import ArrayReader
    rng = np.random.default_rng(4)
    if dst == "rgb":
        frames = [rng.integers(0, 256, size=(3, H, W), dtype=np.uint8) for _ in range(N)]
    else:
        frames = [(rng.integers(0, 256, size=(H, W), dtype=np.uint8),
                   rng.integers(0, 256, size=(2, H // 2, W // 2), dtype=np.uint8)) for _ in range(N)]
    _check_random_access(lambda: ArrayReader(frames), dst)


# ------------------------------------------------------------------ the pool
class _HostLane(L.Lane):
    """A lane that owns no GPU objects: the pool's own logic on host threads."""

    def __init__(self, number):
        super().__init__(number)
        self.drained = 0

    def drain(self):
        self.drained += 1


def _pool(n):
    return L.LanePool([_HostLane(i) for i in range(n)])


@pytest.mark.parametrize("lanes", [1, 2, 3, 8])
def test_pool_returns_frames_in_order(lanes):
    gops = [(0, 4), (4, 5), (5, 16), (16, 19), (19, 23)]
    before = threading.active_count()
    ran = []

    def work(lane, start, stop):
        ran.append((lane.number, start))
        for i in range(start, stop):
            yield (lane.number, i * i)
    out = list(_pool(lanes).run(gops, work))
    assert [i for i, _ in out] == list(range(23)) and all(r[1] == i * i for i, r in out)
    assert sorted(s for _, s in ran) == [g[0] for g in gops]
    assert threading.active_count() == before


def test_pool_bounds_what_waits():
    """GOP g begins only once GOP g - lanes has reached the caller entirely,
    also while GOP 0 is held back until the other lanes have run dry."""
    lanes, gops = 3, L.gop_ranges(40, 4)
    others_done, finished, consumed, begun = threading.Event(), [], [], []

    def work(lane, start, stop):
        g = start // 4
        begun.append((g, len(consumed)))
        if g == 0:
            assert others_done.wait(30)
        try:
            for i in range(start, stop):
                yield i
        finally:                                    # the pool closes a GOP's generator after its last frame
            finished.append(g)
            if {1, 2} <= set(finished):
                others_done.set()
    for i, res in _pool(lanes).run(gops, work):
        assert i == res
        consumed.append(i)
    assert consumed == list(range(40)) and sorted(g for g, _ in begun) == list(range(10))
    for g, seen in begun:
        if g >= lanes:
            assert seen >= gops[g - lanes][1], (g, seen)


def test_pool_lowest_failing_frame_wins():
    gops = L.gop_ranges(16, 4)
    before = threading.active_count()
    later_failed = threading.Event()

    def work(lane, start, stop):
        for i in range(start, stop):
            if i == 9:
                later_failed.set()
                raise KeyError("frame 9")
            if i == 6:
                assert later_failed.wait(30)        # the earlier GOP fails after the later one
                raise ValueError("frame 6")
            yield i
    got = []
    with pytest.raises(ValueError, match="frame 6"):
        for i, _ in _pool(3).run(gops, work):
            got.append(i)
    assert got == [0, 1, 2, 3, 4, 5]
    assert threading.active_count() == before


def test_pool_stops_later_gops_between_frames():
    """After a failure in GOP 0, GOP 1 yields at most the frame it is working
    on and GOPs 2 and 3 never begin."""
    gops = L.gop_ranges(400, 100)
    began0, first, done = threading.Event(), {}, []

    def work(lane, start, stop):
        if start == 0:
            first["thread"] = threading.current_thread()
            began0.set()
        for i in range(start, stop):
            if i == 3:
                raise RuntimeError("frame 3")
            if i == 105:        # until GOP 0's lane has recorded its failure and left
                assert began0.wait(30)
                first["thread"].join(30)
            done.append(i)
            yield i
    with pytest.raises(RuntimeError, match="frame 3"):
        list(_pool(2).run(gops, work))
    assert sorted(done) in ([0, 1, 2], [0, 1, 2] + list(range(100, 106)))


def _count(lane, start, stop):
    yield from range(start, stop)


def test_pool_joins_when_the_caller_stops():
    import contextlib
    before = threading.active_count()
    with contextlib.closing(_pool(3).run(L.gop_ranges(60, 5), _count)) as it:
        assert next(it) == (0, 0)
    assert threading.active_count() == before
    with pytest.raises(ZeroDivisionError), contextlib.closing(_pool(3).run(L.gop_ranges(60, 5), _count)) as it:
        for i, _ in it:
            if i == 7:
                1 / 0
    assert threading.active_count() == before


def test_pool_with_nothing_to_do():
    assert list(_pool(2).run([], _count)) == []


def test_pool_reports_a_failure_after_the_last_frame():
    """A lane that fails in drain(), when every frame has been handed over:
    the frames arrive, then the error is raised and no thread is left."""
    class Leaky(_HostLane):
        def drain(self):
            raise OSError("drain failed")
    before = threading.active_count()
    got = []
    with pytest.raises(OSError, match="drain failed"):
        for i, _ in L.LanePool([Leaky(0), Leaky(1)]).run(L.gop_ranges(12, 4), _count):
            got.append(i)
    assert got == list(range(12))
    assert threading.active_count() == before


def test_pool_drains_every_lane_once():
    lanes = [_HostLane(i) for i in range(3)]
    assert [i for i, _ in L.LanePool(lanes).run(L.gop_ranges(20, 4), _count)] == list(range(20))
    assert [ln.drained for ln in lanes] == [1, 1, 1]

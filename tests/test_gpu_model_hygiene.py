"""Model wiring hygiene: no layer may read a concat channel nobody wrote.

The kernel table (tests/test_gpu_kernel_hygiene.py) cannot see a model that
hands a kernel a view of memory no kernel has written yet.  Here golden
sequence A is coded in split precision through real files three times, on
freshly built nets: with K.empty memory as the allocator hands it back, with
every K.empty activation starting as NaN (hip.POISON = "nan") and as random
bits ("rand"); the two poisoned runs also give every activation a canary tail
(hip.CANARY).  The file bytes, every DPB tensor and the number of precision
fallbacks must not depend on what uninitialised memory held, and no canary
may be overwritten.
"""
import pytest
import torch

from tests.test_gpu_sequence import dc_nets, hem_nets, reference_loop

pytestmark = pytest.mark.gpu

MODES = ("", "nan", "rand")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def coded(kind, make, g, xs, h, w, q, mode, folder):
    """Sequence coded on fresh nets under one poison mode: (frames, canary
    report, fallbacks), frames as reference_loop returns them."""
    from dcvc_amd import hip as K
    old = K.POISON, K.CANARY
    K.POISON, K.CANARY = mode, ([] if mode else None)
    try:
        inet, pnet = make(g)
        frames = reference_loop(kind, inet, pnet, xs, h, w, q, 32, str(folder))
        torch.cuda.synchronize()
        bad = K.check_canaries()
        allocs = len(K.CANARY or [])
    finally:
        K.POISON, K.CANARY = old
    assert not mode or allocs > 100, allocs     # the poisoned runs did go through the canary allocator
    return frames, bad, getattr(inet, "fallbacks", 0) + getattr(pnet, "fallbacks", 0)


def check(kind, make, g, frames_idx, q, tmp_path):
    meta = g.meta["A"]
    h, w = meta["h"], meta["w"]
    xs = [g.frame_tensor("A", t)[1].cuda() for t in frames_idx]
    runs = {}
    for mode in MODES:
        d = tmp_path / (mode or "clean")
        d.mkdir()
        runs[mode] = coded(kind, make, g, xs, h, w, q, mode, d)
    clean, _, clean_fb = runs[""]
    assert clean_fb == 0
    for mode in MODES[1:]:
        frames, bad, fb = runs[mode]
        assert bad == [], (mode, [(s, first) for s, first, _ in bad[:4]])
        assert fb == clean_fb, (mode, fb)
        assert len(frames) == len(clean)
        for t, ((data, dpb, bit), (data0, dpb0, bit0)) in enumerate(zip(frames, clean)):
            assert data == data0 and bit == bit0, (mode, t)
            assert set(dpb) == set(dpb0)
            for k in dpb0:
                if dpb0[k] is None:
                    assert dpb[k] is None, (mode, t, k)
                else:
                    assert not bool(torch.isnan(dpb[k]).any()), (mode, t, k)
                    assert torch.equal(dpb[k], dpb0[k]), (mode, t, k)


def test_dc_sequence_independent_of_uninitialised_memory(dc_golden, tmp_path):
    """DC golden A (176 x 240): I + 2 P."""
    meta = dc_golden.meta["A"]
    assert (meta["h"], meta["w"]) == (176, 240)
    check("dc", dc_nets, dc_golden, range(3), meta["q_index"], tmp_path)


def test_hem_sequence_independent_of_uninitialised_memory(tmp_path):
    """HEM golden A: its three frames."""
    from tests.hem_fixtures import HEMGolden
    g = HEMGolden()
    assert g.meta["A"]["frames"] == 3
    check("hem", hem_nets, g, range(3), g.q("A"), tmp_path)

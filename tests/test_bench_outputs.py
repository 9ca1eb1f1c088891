"""bench.py's plain run, ``--full`` and ``--dump-outputs``: a plain run carries
the headline only (the roofline, CPU baseline and parity check sit behind
--full), --steps sets the number of timed steps, and --dump-outputs writes
what the last timed step returned: float32 / float64 arrays under the size
cap, the bit count being the size of the dumped bitstream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert not a.full and not a.dump_outputs
    assert parse(monkeypatch, "--full").full
    # the per-layer profile comes from the roofline pass, which --full runs
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--profile-out", "x.json")
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--full", "--no-roofline", "--profile-out", "x.json")
    assert parse(monkeypatch, "--full", "--profile-out", "x.json").profile_out == "x.json"


def test_plain_c3_line_keeps_the_metric_name(monkeypatch):
    plain = parse(monkeypatch)
    full = parse(monkeypatch, "--full")
    name = bench.metric_name(full, {"passed": True})
    assert bench.metric_name(plain) == name
    assert "strict GPU test" in bench.parity_evidence(plain, None)
    # not borrowed where no strict test codes the run's own frames
    assert bench.metric_name(parse(monkeypatch, "--q_index", "1")) != name
    assert bench.metric_name(parse(monkeypatch, "--full", "--no-parity-check")) != name
    assert "NOT held" in bench.metric_name(parse(monkeypatch, "--precision", "fast"))


def test_dump_array_formats_and_fixed_sample(tmp_path):
    p = str(tmp_path / "a.npy")
    t = torch.arange(6000, dtype=torch.bfloat16).reshape(1, 3, 40, 50).permute(0, 2, 3, 1)   # a strided view
    bench.dump_array(p, t, 10000)
    a = np.load(p)
    assert a.dtype == np.float32 and np.array_equal(a, t.float().reshape(-1).numpy())
    bench.dump_array(p, t, 500)
    s = np.load(p)
    idx = np.sort(np.random.default_rng(0).integers(0, 6000, 500))
    assert s.dtype == np.float32 and np.array_equal(s, a[idx])
    bench.dump_array(p, b"\x00\x07\xff", 500)
    assert np.array_equal(np.load(p), np.array([0, 7, 255], dtype=np.float32))
    bench.dump_array(p, 123456789, 500)
    assert np.load(p).dtype == np.float64 and np.load(p)[0] == 123456789


@pytest.mark.gpu
def test_plain_run_dumps_last_timed_step(tmp_path):
    """Two lanes, GOP 4, 1 warm-up + 2 timed steps at 100x130: the last timed
    frame is a P-frame, so each lane dumps its DPB and its bitstream."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--height", "100", "--width", "130", "--gop", "4", "--lanes", "2", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["config"]["frames_timed"] == 4 and d["config"]["timed_frames"] == [4, 5]
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["parity_check"] is None
    names = sorted(os.listdir(out))
    assert names == sorted(f"lane{l}_{k}.npy" for l in range(2) for k in
                           ("bit", "bitstream", "dpb_ref_feature", "dpb_ref_frame", "dpb_ref_mv_feature",
                            "dpb_ref_mv_y", "dpb_ref_y"))
    total = 0
    for n in names:
        a = np.load(os.path.join(out, n))
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.size and np.isfinite(a).all(), n
    assert total <= bench.DUMP_BYTES
    for l in range(2):
        bits = np.load(os.path.join(out, f"lane{l}_bit.npy"))
        stream = np.load(os.path.join(out, f"lane{l}_bitstream.npy"))
        # the file's size is the frame's bit count; the lane's total in the line adds the I-frame before it
        assert bits[0] == 8 * stream.size and 0 < bits[0] < d["config"]["bits_per_lane"][l]
        rec = np.load(os.path.join(out, f"lane{l}_dpb_ref_frame.npy"))
        assert rec.size == 3 * 112 * 144 and rec.min() >= 0 and rec.max() <= 1   # whole padded frame, clamped

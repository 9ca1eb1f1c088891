"""Strict, teacher-forced write-mode parity of the DCVC-DC HIP path against the
oracle (tests/parity.py states the bar): every frame is coded by the product
from the ORACLE's decoded picture buffer, so each frame is judged on the same
inputs as the reference, and every differing symbol / index must sit on a
rounding tie of the oracle's own values.

Cases: the golden sequences A (176x240, 4 frames, q 0) and B (100x130, 3
frames, q 40) pinned to the reference by tests/test_oracle_dc.py, and config
C3 at its full size (1920x1080 padded to 1088, I-frame + one P-frame,
q_index 0, the bench's weights and frames).  The decoded picture buffer the
product returns for each frame is compared with the oracle's tensor by tensor
(tests/parity.py: compare_dpb).  Statistics go to
gpurun_out/parity_strict.json.
"""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests.parity import (DPB_FACTOR, REC_MAXABS, REC_MAXABS_HEM, TIE_EPS, check_dpb, check_forced, check_frame,
                          compare_dpb, compare_forced, compare_frame, rec_maxabs, selfnoise)

pytestmark = pytest.mark.gpu

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(16, n)))


def psnr(a, b):
    mse = torch.mean((a.float().cpu() - b.float().cpu()) ** 2)
    return (20 * torch.log10(1 / torch.sqrt(mse))).item()


def _dev(v):
    """A DPB entry for the product: an oracle tensor goes to the GPU, the
    product's own entry (an Act or a GPU tensor) stays as it is."""
    return v.cuda() if torch.is_tensor(v) and not v.is_cuda else v


class Pair:
    """Oracle and product codecs built from the same state dicts
    (``product=False``: the oracle alone, which needs no GPU)."""

    def __init__(self, i_sd, p_sd, prec="parity", stream_part=1, ec_thread=False, product=True):
        from oracle import dc_oracle as O
        from oracle import rans_oracle as R
        self.R = R
        self.parts = stream_part
        self.prec = prec
        self.oi = O.IntraOracle(i_sd, R.pmf_to_quantized_cdf)
        self.op = O.DMCOracle(p_sd, R.pmf_to_quantized_cdf)
        self.tabs = {"i_y": (self.oi.y_cdf, self.oi.y_sizes, self.oi.y_offsets), "i_z": self.oi.z_tab,
                     "p_y": (self.op.y_cdf, self.op.y_sizes, self.op.y_offsets), "p_z": self.op.z_tab,
                     "p_mvz": self.op.mvz_tab}
        if not product:
            return
        from dcvc_amd.dc import DMC, IntraNoAR
        from dcvc_amd.layers import Precision
        P = getattr(Precision, prec)
        # the coder configuration of the reference's --ec_thread /
        # --stream_part_{i,p} options (test_video.py:29-31), the bench's 8
        # parts on worker threads included
        kw = dict(stream_part=stream_part, ec_thread=ec_thread)
        self.pi = IntraNoAR(precision=P(), **kw).load_state_dict(i_sd)
        self.pp = DMC(precision=P(), **kw).load_state_dict(p_sd)
        self.pi.update(force=True)
        self.pp.update(force=True)

    def oracle(self, t, xp, dpb, q, fidx, force=None):
        tap = {}
        with torch.no_grad():
            if t == 0:
                calls, xh = self.oi.compress(xp, False, q, tap=tap, recon=True, force=force)
                dpb = {"ref_frame": xh, "ref_feature": None, "ref_mv_feature": None, "ref_y": None, "ref_mv_y": None}
            else:
                calls, dpb = self.op.compress(xp, dpb, False, q, fidx, tap=tap, recon=True, force=force)
        pre = "i_" if t == 0 else "p_"
        cc = [(s.clamp(-30000, 30000).to(torch.int16).numpy(), ix.to(torch.int16).numpy(), self.tabs[pre + k])
              for k, s, ix in calls]
        stream = self.R.DCStream(self.parts).encode(cc)
        return calls, tap, (len(stream) + (13 if t == 0 else 6)) * 8, dpb

    def coded_bits(self, t, calls):
        """Bits of a frame's calls [(kind, symbols, indexes)] through the
        oracle's coder, with the stream headers encode_i / encode_p add."""
        pre = "i_" if t == 0 else "p_"
        cc = [(np.clip(np.asarray(s).reshape(-1).astype(np.int64), -30000, 30000).astype(np.int16),
               np.asarray(ix).reshape(-1).astype(np.int16), self.tabs[pre + k]) for k, s, ix in calls]
        return (len(self.R.DCStream(self.parts).encode(cc)) + (13 if t == 0 else 6)) * 8

    def product(self, t, xp, dpb_o, q, fidx, path, h, w, want_dpb=False):
        """``dpb_o``: the oracle's DPB (CPU tensors) or the product's own, as
        a former call returned it with ``want_dpb`` (a fourth value)."""
        net = self.pi if t == 0 else self.pp
        net.entropy_coder.trace = []
        if t == 0:
            r = self.pi.encode_decode(xp.cuda(), False, q, path, pic_width=w, pic_height=h)
            rec = r["x_hat"]
            dpb_p = {"ref_frame": rec, "ref_feature": None, "ref_mv_feature": None, "ref_y": None, "ref_mv_y": None}
        else:
            dpb = {k: _dev(v) for k, v in dpb_o.items()}
            r = self.pp.encode_decode(xp.cuda(), dpb, False, q, path, pic_width=w, pic_height=h, frame_idx=fidx)
            dpb_p = r["dpb"]
            rec = dpb_p["ref_frame"]
        tr = net.entropy_coder.trace
        net.entropy_coder.trace = None
        enc = [(s, i) for k, s, i in tr if k == "enc"]
        dec = [(s, i) for k, s, i in tr if k == "dec"]
        assert len(enc) == len(dec)
        for (se, ie), (sd, id_) in zip(enc, dec):   # lossless: the decoder reads what the encoder wrote
            np.testing.assert_array_equal(ie.reshape(-1), id_.reshape(-1))
            np.testing.assert_array_equal(se.reshape(-1), sd.reshape(-1))
        return (enc, r["bit"], rec.clamp(0, 1)) + ((dpb_p,) if want_dpb else ())


def run_teacher_forced(pair, frames, q, h, w, name):
    """frames: [(x (1,3,h,w), xp padded)]; frame t > 0 is coded from the
    oracle's dpb of frame t-1.  The DPB the product returns is held to the
    bar of the free-running cases (tests/parity.py: the oracle's recorded
    self-noise of DC-bench / HEM-bench times the precision's factor) against
    the oracle's, or the replay's after a flipped tie.  hem_C1 is held to the
    oracle's self-noise on its own frames (HEM-C1 of the fixture; ref_mv_y,
    which those runs leave unmeasured, to HEM-bench's): on C1's torch.rand
    frames the oracle at another thread count alone takes 0.7-0.8 of the
    HEM-bench bar in ref_frame, and the fp32 product 0.99 of it (DESIGN.md
    section 5.4 has the layer table), so that bar was decided by the host CPU."""
    stats, dpb_o = [], None
    rec_bar = REC_MAXABS_HEM if name.startswith("hem") else REC_MAXABS
    if name.startswith("hem_C1"):
        noise = selfnoise("HEM-C1", unmeasured="HEM-bench")
    else:
        noise = selfnoise("HEM-bench" if name.startswith("hem") else "DC-bench")
    factor = DPB_FACTOR[pair.prec]
    with tempfile.TemporaryDirectory() as td:
        for t, (x, xp) in enumerate(frames):
            fidx = t % 4
            calls, tap, bits_o, dpb_next = pair.oracle(t, xp, dpb_o, q, fidx)
            enc, bits, rec, dpb_p = pair.product(t, xp, dpb_o, q, fidx, os.path.join(td, f"{t}.bin"), h, w,
                                                 want_dpb=True)
            st = compare_frame(enc, calls, tap)
            p = psnr(rec[:, :, :h, :w], x)
            p_o = psnr(dpb_next["ref_frame"][:, :, :h, :w], x)
            st.update({"t": t, "bits": int(bits), "bits_oracle": int(bits_o), "psnr": p, "psnr_oracle": p_o,
                       "rec_maxabs": rec_maxabs(rec[:, :, :h, :w], dpb_next["ref_frame"][:, :, :h, :w].clamp(0, 1))})
            msg = check_frame(st, bits, bits_o, p, p_o, f"{name} t={t}", rec_bar)
            dpb_ref = dpb_next
            if st["sym_diff"]:
                # the cascade after a flipped tie, element by element: the
                # oracle replays the product's symbols at its ties and runs the
                # rest of the frame on the product's y_hat
                from oracle.dc_oracle import Forcer
                fr = Forcer([s for s, _ in enc], TIE_EPS)
                calls_f, tap_f, bits_f, dpb_f = pair.oracle(t, xp, dpb_o, q, fidx, force=fr)
                sf = compare_forced(enc, calls_f, tap_f, fr.forced)
                p_f = psnr(dpb_f["ref_frame"][:, :, :h, :w], x)
                sf.update({"bits_replay": int(bits_f), "psnr_replay": p_f,
                           "rec_maxabs": rec_maxabs(rec[:, :, :h, :w], dpb_f["ref_frame"][:, :, :h, :w].clamp(0, 1))})
                if sf["sym_diff"] == 0:
                    # every symbol agrees and every differing index is a tie
                    # of the replay (compare_forced): the replay's stream with
                    # the product's index at those ties must be the product's
                    # stream, to the bit
                    sf["bits_replay_tied"] = pair.coded_bits(
                        t, [(c[0], ps, pi) for c, (ps, pi) in zip(calls_f, enc)])
                st["replay"] = sf
                msg += "\n" + check_forced(sf, bits, bits_f, p, p_f, f"{name} t={t}", rec_bar)
                dpb_ref = dpb_f
            st["dpb"] = compare_dpb(dpb_p, dpb_ref, h, w, noise, factor)
            msg += f"\n{name} t={t} DPB rel / bar: " + ", ".join(
                f"{k} {v['ratio']:.3g}" for k, v in st["dpb"].items())
            stats.append((st, msg))
            dpb_o = dpb_next
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "parity_strict.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d[name] = [s for s, _ in stats]
    json.dump(d, open(path, "w"), indent=1)
    for t, (st, _) in enumerate(stats):   # after the record is written
        check_dpb(st["dpb"], f"{name} t={t}")
    return stats


PRECS = ["split", "parity"]   # split = the bench's precision (split-fp16 MFMA), parity = fp32 MFMA


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", ["A", "B"])
def test_strict_parity_golden(dc_golden, tag, prec):
    meta = dc_golden.meta[tag]
    pair = Pair(dc_golden.i_state_dict(), dc_golden.p_state_dict(), prec)
    frames = [dc_golden.frame_tensor(tag, t) for t in range(meta["frames"])]
    stats = run_teacher_forced(pair, frames, meta["q_index"], meta["h"], meta["w"], f"golden_{tag}_{prec}")
    for st, msg in stats:
        print(msg)


@pytest.mark.parametrize("prec", PRECS)
def test_strict_parity_c3_1080p(prec):
    """Config C3 at full size: I-frame + P-frame (frame_idx 1), q_index 0."""
    import bench
    from dcvc_amd.synth import moving_pattern, to_float
    isd, psd = bench.make_weights(None, 0, torch.device("cpu"), "dc")
    h, w = 1080, 1920
    frames = []
    for t in range(2):
        x = torch.from_numpy(to_float(moving_pattern(h, w, t, seed=1))).unsqueeze(0)
        frames.append((x, torch.nn.functional.pad(x, (0, 0, 0, 8), mode="replicate")))
    pair = Pair(isd, psd, prec)
    stats = run_teacher_forced(pair, frames, 0, h, w, f"C3_1080p_{prec}")
    for st, msg in stats:
        print(msg)


@pytest.mark.parametrize("case", ["golden_A", "C3_1080p"])
def test_strict_parity_multipart_threaded(dc_golden, case):
    """The bench's coder configuration: DC streams in 8 parts coded on worker
    threads (stream_part 8, ec_thread True; DCVC-DC/src/cpp/py_rans/
    py_rans.cpp:11-225, test_video.py:29-31), in the bench's split precision,
    held to the strict bar against the oracle's coder at the same part count
    (golden A, and C3 at full size: I-frame + P-frame)."""
    if case == "golden_A":
        meta = dc_golden.meta["A"]
        pair = Pair(dc_golden.i_state_dict(), dc_golden.p_state_dict(), "split", stream_part=8, ec_thread=True)
        frames = [dc_golden.frame_tensor("A", t) for t in range(meta["frames"])]
        q, h, w = meta["q_index"], meta["h"], meta["w"]
    else:
        import bench
        from dcvc_amd.synth import moving_pattern, to_float
        isd, psd = bench.make_weights(None, 0, torch.device("cpu"), "dc")
        h, w, q = 1080, 1920, 0
        frames = []
        for t in range(2):
            x = torch.from_numpy(to_float(moving_pattern(h, w, t, seed=1))).unsqueeze(0)
            frames.append((x, torch.nn.functional.pad(x, (0, 0, 0, 8), mode="replicate")))
        pair = Pair(isd, psd, "split", stream_part=8, ec_thread=True)
    stats = run_teacher_forced(pair, frames, q, h, w, f"{case}_split_parts8_threaded")
    for st, msg in stats:
        print(msg)


@pytest.mark.parametrize("prec", PRECS)
def test_strict_parity_c3small_survey_recipe(prec):
    """The survey's C3-small recipe (default-init weights, 4 torch.rand 256x256
    frames, q_index 0): strict parity against the oracle, and on every frame
    whose calls all agree, the survey's recorded bits exactly."""
    from tests.test_oracle_c3small import C3Small
    c3s = C3Small()
    frames = [(x, x) for x in c3s.frames()]
    pair = Pair(c3s.i_sd, c3s.p_sd, prec)
    stats = run_teacher_forced(pair, frames, 0, 256, 256, f"C3small_survey_{prec}")
    for (st, msg), want in zip(stats, c3s.meta["survey_bits"]):
        print(msg)
        if st["identical"]:
            assert st["bits"] == want, msg


# (h, w, frames): I + P at 1080p and at C4's own 3840x2160 (latent grid
# 135x240, hyperprior pad to 136x240, 4K tile counts; the oracle takes about a
# minute per 4K I-frame on 16 host threads and three per P-frame)
C4_SIZES = {"1080p": (1080, 1920, 2), "2160p": (2160, 3840, 2)}


@pytest.mark.parametrize("size", ["1080p", "2160p"])
@pytest.mark.parametrize("prec", ["split"])
def test_strict_parity_c4_yuv420(prec, size):
    """The C4 path (DCVC-DC on YUV420 input, test_video.py:110-195 with
    src_type yuv420: 4:2:0 planes upsampled to 4:4:4 YCbCr and padded to a
    multiple of 16 on the GPU; 2160 and 3840 need none) in the bench's split
    precision: the GPU-converted input equals the oracle's conversion bit for
    bit, then the frames are held to the strict bar, at 1080p and at C4's own
    3840x2160 (DCVC-DC/src/models/common_model.py:70-86: pad_for_y /
    slice_to_y of the 135x240 latent grid)."""
    import bench
    from dcvc_amd.harness import FrameStage
    from dcvc_amd.synth import moving_pattern_yuv420
    from oracle.harness_oracle import yuv_u8_to_input
    isd, psd = bench.make_weights(None, 0, torch.device("cpu"), "dc")
    h, w, nf = C4_SIZES[size]
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    dev = torch.device("cuda", 0)
    stage = FrameStage(h, w, 16, True, zero_pad=False, frame_num=nf, device=dev)
    frames = []
    for t in range(nf):
        y, uv = moving_pattern_yuv420(h, w, t, seed=1)
        xo = torch.from_numpy(yuv_u8_to_input(y, uv, H, W)).permute(2, 0, 1).unsqueeze(0).contiguous()
        xg = stage.load((torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev)))
        xg = xg.nchw() if hasattr(xg, "nchw") else xg
        assert torch.equal(xg.float().cpu(), xo), "GPU YUV420 -> 4:4:4 input differs from the oracle's"
        frames.append((xo[:, :, :h, :w], xo))
        del xg
    pair = Pair(isd, psd, prec)
    name = f"C4path_yuv420_1080p_{prec}" if size == "1080p" else f"C4_yuv420_2160p_{prec}"
    stats = run_teacher_forced(pair, frames, 0, h, w, name)
    for st, msg in stats:
        print(msg)


class HemPair(Pair):
    """DCVC-HEM: oracle/hem_oracle.py and dcvc_amd.hem in parity precision;
    one headerless int32 stream per frame (the reference's
    BufferedRansEncoder), coded here by the oracle's C restatement."""

    def __init__(self, i_sd, p_sd, q, prec="parity", product=True):
        from oracle import hem_oracle as O
        from oracle import rans_oracle as R
        self.O, self.R = O, R
        self.q = q
        self.prec = prec
        self.oi = O.IntraOracle(i_sd, R.pmf_to_quantized_cdf)
        self.op = O.DMCOracle(p_sd, R.pmf_to_quantized_cdf)
        self.tabs = {"i_y": self.oi.tab_y[:3], "i_z": self.oi.tab_z[:3], "p_y": self.op.tab_y[:3],
                     "p_z": self.op.tab_z[:3], "p_mvz": self.op.tab_mvz[:3]}
        if not product:
            return
        from dcvc_amd.hem import DMC, IntraNoAR
        from dcvc_amd.layers import Precision
        P = getattr(Precision, prec)
        self.pi = IntraNoAR(precision=P()).load_state_dict(i_sd)
        self.pp = DMC(precision=P()).load_state_dict(p_sd)
        self.pi.update(force=True)
        self.pp.update(force=True)

    def _stream_bytes(self, calls):
        """All calls of a frame through one coder state (one stream)."""
        names = sorted({k for k, _, _ in calls})
        stride = max(self.tabs[n][0].shape[1] for n in names)
        base, rows, r = {}, [], 0
        for n in names:
            c = np.asarray(self.tabs[n][0])
            base[n] = r
            rows.append(np.pad(c, ((0, 0), (0, stride - c.shape[1]))))
            r += c.shape[0]
        cdfs = np.concatenate(rows).astype(np.int32)
        sizes = np.concatenate([np.asarray(self.tabs[n][1]).reshape(-1) for n in names]).astype(np.int32)
        offs = np.concatenate([np.asarray(self.tabs[n][2]).reshape(-1) for n in names]).astype(np.int32)
        sym = np.concatenate([s.reshape(-1) for _, s, _ in calls]).astype(np.int32)
        idx = np.concatenate([i.reshape(-1).astype(np.int32) + base[k] for k, _, i in calls])
        return len(self.R.hem_encode(sym, idx, cdfs, sizes, offs))

    def oracle(self, t, xp, dpb, q, fidx, force=None):
        O = self.O
        qi, qmv, qy = (round(v * 100) / 100 for v in self.q)
        tap = {}
        with torch.no_grad():
            if t == 0:
                calls, xh = self.oi.compress(xp, qi, tap=tap, recon=True, force=force)
                dpb = {"ref_frame": xh, "ref_feature": None, "ref_y": None, "ref_mv_y": None}
            else:
                calls, dpb = self.op.compress(xp, dpb, qmv, qy, tap=tap, recon=True, force=force)
        net = self.oi if t == 0 else self.op
        out = []
        for kind, sym, sc in calls:
            if sc is None:
                C, h, w = sym.shape[1:]
                idx = O.channel_indexes(C, h, w)
            else:
                idx = O.build_indexes(sc, net.tab_y[3], net.tab_y[4]).reshape(-1)
            out.append((kind, sym.reshape(-1), idx))
        nbytes = self._stream_bytes([(k, s.int().numpy(), i.numpy()) for k, s, i in out])
        return out, tap, (nbytes + (14 if t == 0 else 8)) * 8, dpb

    def coded_bits(self, t, calls):
        return (self._stream_bytes([(k, np.asarray(s).astype(np.int32), np.asarray(i)) for k, s, i in calls])
                + (14 if t == 0 else 8)) * 8

    def product(self, t, xp, dpb_o, q, fidx, path, h, w, want_dpb=False):
        qi, qmv, qy = self.q
        net = self.pi if t == 0 else self.pp
        net.entropy_coder.trace = []
        if t == 0:
            r = self.pi.encode_decode(xp.cuda(), qi, path, pic_width=w, pic_height=h)
            rec = r["x_hat"]
            dpb_p = {"ref_frame": rec, "ref_feature": None, "ref_y": None, "ref_mv_y": None}
        else:
            dpb = {k: _dev(v) for k, v in dpb_o.items()}
            r = self.pp.encode_decode(xp.cuda(), dpb, path, pic_width=w, pic_height=h, mv_y_q_scale=qmv,
                                      y_q_scale=qy)
            dpb_p = r["dpb"]
            rec = dpb_p["ref_frame"]
        tr = net.entropy_coder.trace
        net.entropy_coder.trace = None
        enc = [(s, i) for k, s, i in tr if k == "enc"]
        dec = [(s, i) for k, s, i in tr if k == "dec"]
        assert len(enc) == len(dec)
        for (se, ie), (sd, id_) in zip(enc, dec):
            np.testing.assert_array_equal(ie.reshape(-1), id_.reshape(-1))
            np.testing.assert_array_equal(se.reshape(-1), sd.reshape(-1))
        return (enc, r["bit"], rec.clamp(0, 1)) + ((dpb_p,) if want_dpb else ())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", ["C1", "A", "B"])
def test_strict_parity_hem(tag, prec):
    """DCVC-HEM: config C1 (4 random 256x256 frames, IP=4; write mode codes
    I, P1, P2 as the survey's recipe) and the golden sequences A, B."""
    from tests.hem_fixtures import HEMGolden
    g = HEMGolden()
    meta = g.meta[tag]
    pair = HemPair(g.i_state_dict(), g.p_state_dict(), g.q(tag), prec)
    frames = [g.frame_tensor(tag, t) for t in range(g.write_frames(tag))]
    stats = run_teacher_forced(pair, frames, None, meta["h"], meta["w"], f"hem_{tag}_{prec}")
    for st, msg in stats:
        print(msg)


@pytest.mark.parametrize("prec", ["split"])
def test_strict_parity_hem_c2_1080p(prec):
    """Config C2 at full size (DCVC-HEM, 1920x1080 zero-padded to 1088, the
    bench's weights, frames and rate point 0): I-frame + P-frame, teacher
    forced, in the bench's split precision."""
    import bench
    from dcvc_amd.synth import moving_pattern, to_float
    isd, psd = bench.make_weights(None, 0, torch.device("cpu"), "hem")
    h, w = 1080, 1920
    frames = []
    for t in range(2):
        x = torch.from_numpy(to_float(moving_pattern(h, w, t, seed=1))).unsqueeze(0)
        frames.append((x, torch.nn.functional.pad(x, (0, 0, 0, 8), mode="constant", value=0)))
    pair = HemPair(isd, psd, bench.hem_q(isd, psd, 0), prec)
    stats = run_teacher_forced(pair, frames, None, h, w, f"hem_C2_1080p_{prec}")
    for st, msg in stats:
        print(msg)


@pytest.mark.parametrize("prec", PRECS)
def test_hem_c1_estimate_teacher_forced(prec):
    """Config C1 in estimate mode (encode_decode(output_path=None), all four
    frames, IP=4): each P-frame from the oracle's dpb (the oracle reproduces
    the reference's estimate mode bit for bit, tests/test_oracle_hem.py);
    bits against the reference's own estimates, PSNR against the oracle's."""
    from tests.hem_fixtures import HEMGolden
    g = HEMGolden()
    meta = g.meta["C1"]
    pair = HemPair(g.i_state_dict(), g.p_state_dict(), g.q("C1"), prec)
    qi, qmv, qy = g.q("C1")
    dpb_o, rows = None, []
    # the fixture's estimates were made at 8 CPU threads; the oracle runs at
    # that count too, but its float sums also follow the CPU's vector width, so
    # on another machine a rounding tie can still fall the other way: on the
    # GPU box frame 2's oracle estimate sat 4.1e-4 from the reference's and
    # frame 3's reference 3.0e-4 from the oracle's
    nthr = torch.get_num_threads()
    torch.set_num_threads(8)
    with torch.no_grad():
        for t in range(meta["frames"]):
            x, xp = g.frame_tensor("C1", t)
            if t == 0:
                bit_o, xh = pair.oi.forward(xp, qi)
                nxt = {"ref_frame": xh, "ref_feature": None, "ref_y": None, "ref_mv_y": None}
                r = pair.pi.encode_decode(xp.cuda(), qi)
                rec = r["x_hat"]
            else:
                bit_o, nxt = pair.op.forward_one_frame(xp, dpb_o, qmv, qy)
                dpb = {k: (v.cuda() if v is not None else None) for k, v in dpb_o.items()}
                r = pair.pp.encode_decode(xp.cuda(), dpb, mv_y_q_scale=qmv, y_q_scale=qy)
                rec = r["dpb"]["ref_frame"]
            nxt["ref_frame"].clamp_(0, 1)
            ref_bit = meta["est"][t]["bit"]
            # the oracle reproduces the reference's estimate bit for bit at the
            # fixture's 8 threads (tests/test_oracle_hem.py); at another thread
            # count the CPU's own float sums move a rounding tie now and then,
            # which changes its dpb and the later frames' estimates: the product
            # is judged against the oracle on the oracle's dpb, the reference's
            # number is reported beside it
            p = psnr(rec.clamp(0, 1), x)
            p_o = psnr(nxt["ref_frame"], x)
            rows.append({"t": t, "bit": float(r["bit"]), "bit_oracle": float(bit_o), "bit_ref": ref_bit, "psnr": p,
                         "psnr_oracle": p_o})
            dpb_o = nxt
    torch.set_num_threads(nthr)
    print(rows)
    for s in rows:
        # estimated bits are sums of -log2 p over every element: a symbol or
        # index flipped at a rounding tie (the ties tests/parity.py admits)
        # moves a frame's estimate by a few bits to tens of bits (3e-5 of it
        # seen in split precision).  The product must sit within 1e-4 of one
        # of the two CPU computations of the frame, the oracle's or the
        # reference's own (which differ at such ties by up to 4e-4, above);
        # measured: within 2e-7 of one of them on every frame
        d = min(abs(s["bit"] - s["bit_oracle"]), abs(s["bit"] - s["bit_ref"]))
        assert d / s["bit_ref"] < 1e-4, s
        assert abs(s["bit_oracle"] - s["bit_ref"]) / s["bit_ref"] < 1e-3, s
        assert abs(s["psnr"] - s["psnr_oracle"]) < 1e-4, s

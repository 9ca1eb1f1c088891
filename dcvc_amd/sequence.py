"""One coded video in one file, written by an encoder that never decodes and
read by a decoder that never encodes (INTEGRATION.md "Sequence file").

``SequenceWriter`` / ``SequenceReader`` are the host side (no GPU): a header
that says which codec, format and precision wrote the file, then one record
per frame with its type, flags, the DPB digest and the unmodified
reference-format frame bytes (``stream_helper.pack_i`` / ``pack_p``).

``SequenceEncoder`` / ``SequenceDecoder`` drive the codecs' ``encode_frame`` /
``decode_frame``.  Each keeps its own decoded picture buffer from frame to
frame; the encoder stores a digest of it per frame (``hip.digest`` folded over
the DPB tensors) and the decoder compares its own, so any difference between
the two sides stops the decode at the first frame it touches instead of
drifting through the GOP.

``python -m dcvc_amd.sequence encode|decode ...`` wraps
``harness.encode_video`` / ``decode_video``.
"""
import collections
import os
import struct

import torch

MAGIC = b"DCVCSEQ1"
CODECS = ("DC", "HEM")
FORMATS = ("rgb", "yuv420")
NOT_CLOSED = 0xFFFFFFFF
FLAG_TWIN, FLAG_DIGEST = 1, 2
_HEADER = struct.Struct("<8sBB16sHIII")     # magic, codec, format, precision, bit depth, width, height, frames
_RECORD = struct.Struct("<BBHIQQ")          # type, flags, reserved, payload length, digest S, digest X
_COUNT_AT = _HEADER.size - 4
# seeds of the frame digest, by DPB entry (an I frame: x_hat under seed 1)
DIGEST_SEEDS = (("ref_frame", 1), ("ref_feature", 2), ("ref_mv_feature", 3), ("ref_y", 4), ("ref_mv_y", 5))


# one frame of SequenceReader.index(): where its payload lies in the file
IndexEntry = collections.namedtuple("IndexEntry", "frame_idx type flags offset length")


class SequenceFormatError(ValueError):
    """Not a sequence file, or one that is truncated or was never closed."""


class DigestMismatch(RuntimeError):
    """The decoder's DPB after a frame is not the encoder's."""

    def __init__(self, frame_idx, stored, computed):
        self.frame_idx, self.stored, self.computed = frame_idx, tuple(stored), tuple(computed)
        super().__init__(f"frame {frame_idx}: the stream stores DPB digest ({stored[0]:#018x}, {stored[1]:#018x}), "
                         f"this decoder computed ({computed[0]:#018x}, {computed[1]:#018x})")


# ---------------------------------------------------------------- the file
def header_bit_depth(bit_depth):
    """The header's bit-depth field for a source of ``bit_depth`` bits: 0
    (8 bits / unspecified, what every 8-bit encode writes) or 9..16."""
    if bit_depth not in (0,) + tuple(range(8, 17)):
        raise ValueError(f"bit depth {bit_depth!r} is not 0 or 8..16")
    return 0 if bit_depth == 8 else bit_depth


class SequenceWriter:
    def __init__(self, path, codec, fmt, precision, width, height, bit_depth=0):
        if codec not in CODECS or fmt not in FORMATS:
            raise ValueError(f"unknown codec / format {codec!r} / {fmt!r}")
        field = header_bit_depth(bit_depth)
        name = precision.encode("ascii")
        if not 0 < len(name) <= 16:
            raise ValueError(f"precision name {precision!r} does not fit 16 bytes")
        self.frames = 0
        self.file = open(path, "wb")  # noqa: SIM115 (closed in close())
        self.file.write(_HEADER.pack(MAGIC, CODECS.index(codec), FORMATS.index(fmt), name, field, width, height,
                                     NOT_CLOSED))

    def write(self, frame_type, payload, twin=False, digest=None):
        if frame_type not in ("I", "P"):
            raise ValueError(f"unknown frame type {frame_type!r}")
        flags = (FLAG_TWIN if twin else 0) | (FLAG_DIGEST if digest is not None else 0)
        s, x = digest if digest is not None else (0, 0)
        self.file.write(_RECORD.pack("IP".index(frame_type), flags, 0, len(payload), s, x))
        self.file.write(payload)
        self.frames += 1

    def close(self):
        """Patch the frame count in; a file without it counts as unfinished."""
        if self.file is None:
            return
        self.file.seek(_COUNT_AT)
        self.file.write(struct.pack("<I", self.frames))
        self.file.close()
        self.file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class SequenceReader:
    """Header fields as attributes (codec, format, precision, bit_depth (the
    source's, 8 for a field of 0), width, height, frames); iterating yields
    {"type", "twin", "digest" (or None), "payload"}.  ``index()`` and
    ``records_from()`` give random access by frame."""

    def __init__(self, path):
        self.path = path
        self.file = open(path, "rb")  # noqa: SIM115 (closed in close())
        head = self.file.read(_HEADER.size)
        if len(head) < _HEADER.size or head[:8] != MAGIC:
            self.close()
            raise SequenceFormatError(f"{path}: not a {MAGIC.decode()} sequence file")
        _, codec, fmt, name, depth, self.width, self.height, self.frames = _HEADER.unpack(head)
        if codec >= len(CODECS) or fmt >= len(FORMATS):
            self.close()
            raise SequenceFormatError(f"{path}: unknown codec / format code {codec} / {fmt}")
        if depth != 0 and not 8 <= depth <= 16:
            self.close()
            raise SequenceFormatError(f"{path}: source bit depth {depth} is not 0 or 8..16")
        self.bit_depth = depth or 8
        self.codec, self.format = CODECS[codec], FORMATS[fmt]
        self.precision = name.rstrip(b"\0").decode("ascii")
        if self.frames == NOT_CLOSED:
            self.close()
            raise SequenceFormatError(f"{path}: the file was not closed by its encoder (no frame count)")

    def index(self):
        """One ``IndexEntry`` per frame, from a walk over the 24-byte record
        headers that seeks over every payload and reads none.  The file stores
        no index; this rebuilds it.  The sequential cursor is left where it
        was."""
        size = os.fstat(self.file.fileno()).st_size
        keep = self.file.tell()
        entries, pos = [], _HEADER.size
        try:
            for i in range(self.frames):
                self.file.seek(pos)
                head = self.file.read(_RECORD.size)
                if len(head) < _RECORD.size:
                    raise SequenceFormatError(f"{self.path}: truncated in the record header of frame {i}")
                ftype, flags, _, n, _, _ = _RECORD.unpack(head)
                if ftype > 1:
                    raise SequenceFormatError(f"{self.path}: frame {i} has unknown type {ftype}")
                pos += _RECORD.size
                if pos + n > size:
                    raise SequenceFormatError(f"{self.path}: truncated in the payload of frame {i} "
                                              f"({max(size - pos, 0)} of {n} bytes)")
                entries.append(IndexEntry(i, "IP"[ftype], flags, pos, n))
                pos += n
        finally:
            self.file.seek(keep)
        return entries

    def records_from(self, entry, count=None):
        """The records from ``entry`` (one of ``index()``) on, ``count`` of
        them or up to the end of the file, as iterating yields them."""
        self.file.seek(entry.offset - _RECORD.size)
        stop = self.frames if count is None else min(self.frames, entry.frame_idx + count)
        return self._records(entry.frame_idx, stop)

    def __iter__(self):
        return self._records(0, self.frames)

    def _records(self, first, stop):
        for i in range(first, stop):
            head = self.file.read(_RECORD.size)
            if len(head) < _RECORD.size:
                raise SequenceFormatError(f"{self.path}: truncated in the record header of frame {i}")
            ftype, flags, _, n, s, x = _RECORD.unpack(head)
            if ftype > 1:
                raise SequenceFormatError(f"{self.path}: frame {i} has unknown type {ftype}")
            payload = self.file.read(n)
            if len(payload) < n:
                raise SequenceFormatError(f"{self.path}: truncated in the payload of frame {i} "
                                          f"({len(payload)} of {n} bytes)")
            yield {"type": "IP"[ftype], "twin": bool(flags & FLAG_TWIN),
                   "digest": (s, x) if flags & FLAG_DIGEST else None, "payload": payload}

    def close(self):
        if self.file is not None:
            self.file.close()
            self.file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# -------------------------------------------------------------- the drivers
def codec_of(net):
    return "HEM" if type(net).__module__.startswith("dcvc_amd.hem") else "DC"


def _describe(i_net, p_net):
    """(codec, format, precision name) of a pair of nets.  The format is the
    nets' ``codec_format`` attribute ("rgb" unless the caller, who knows which
    checkpoint they hold, set "yuv420")."""
    codec = codec_of(i_net)
    if codec_of(p_net) != codec:
        raise ValueError("the I and the P codec are not of one family (DC / HEM)")
    fmt = getattr(i_net, "codec_format", "rgb")
    if getattr(p_net, "codec_format", "rgb") != fmt or fmt not in FORMATS:
        raise ValueError("the I and the P codec do not carry one codec_format (rgb / yuv420)")
    if i_net.prec.name != p_net.prec.name:
        raise ValueError(f"the I codec runs in {i_net.prec.name} precision, the P codec in {p_net.prec.name}")
    return codec, fmt, i_net.prec.name


class FrameDigest:
    """The frame digest: ``hip.digest`` folded over the DPB entries in the
    order and under the seeds of DIGEST_SEEDS, all on the current stream; one
    16-byte transfer (which waits for them) returns the two words."""

    def __init__(self, device):
        self.out = torch.zeros(2, dtype=torch.int64, device=device)

    def __call__(self, dpb):
        from . import hip as K
        from .dc.video_model import as_act
        self.out.zero_()
        for name, seed in DIGEST_SEEDS:
            t = dpb.get(name)
            if t is None:
                continue
            if isinstance(t, torch.Tensor) and t.dim() == 3:      # an (H, W, C) copy of an entry
                t = K.Act(t.contiguous())
            K.digest(as_act(t), seed, self.out)
        s, x = self.out.cpu().tolist()
        return s & 0xFFFFFFFFFFFFFFFF, x & 0xFFFFFFFFFFFFFFFF


def _i_dpb(codec, x_hat):
    dpb = {"ref_frame": x_hat, "ref_feature": None, "ref_y": None, "ref_mv_y": None}
    if codec == "DC":
        dpb["ref_mv_feature"] = None
    return dpb


class SequenceEncoder:
    """Encoder only.  ``encode(x)`` takes the padded codec input of one frame
    (what ``FrameStage.load`` produces), codes it against the encoder's own
    DPB, appends the record and returns the codec's ``encode_frame`` dict plus
    "type", "recon" (the (1, 3, H, W) reconstruction) and "digest".  The I/P
    schedule, the P codec's q and ``frame_idx`` are those of ``run_test`` /
    ``run_test_hem``: DC passes (q_in_ckpt, q_index) to both codecs and
    ``frame_idx % 4``; HEM passes i_frame_q_scale and the two P scales.
    ``encode(x, keyframe=True)`` asks for an I frame out of turn (a scene cut):
    the ``scenecut.KeyframeSchedule`` grants it once ``min_keyframe_interval``
    frames have passed since the last keyframe and counts ``gop_size`` from it
    again.  The DC P codec keeps the global ``frame_idx % 4`` (the decoder
    reads it from the payload).
    ``bit_depth`` is the source's, for the header only: no payload depends on it."""

    def __init__(self, i_net, p_net, path, width, height, gop_size, q_in_ckpt=False, q_index=None,
                 i_frame_q_scale=None, p_frame_mv_y_q_scale=None, p_frame_y_q_scale=None, yuv420=False, digest=True,
                 bit_depth=8, min_keyframe_interval=1):
        from .scenecut import KeyframeSchedule
        self.codec, fmt, prec = _describe(i_net, p_net)
        if fmt != FORMATS[int(bool(yuv420))]:
            raise ValueError(f"the nets carry codec_format {fmt!r}, the caller asks for {FORMATS[int(bool(yuv420))]!r}")
        if self.codec == "DC" and q_index is None:
            raise ValueError("the DC codecs need q_index")
        if self.codec == "HEM" and None in (i_frame_q_scale, p_frame_mv_y_q_scale, p_frame_y_q_scale):
            raise ValueError("the HEM codecs need i_frame_q_scale, p_frame_mv_y_q_scale and p_frame_y_q_scale")
        self.i_net, self.p_net = i_net, p_net
        self.width, self.height, self.gop_size = width, height, gop_size
        self.q = (q_in_ckpt, q_index) if self.codec == "DC" else (i_frame_q_scale, p_frame_mv_y_q_scale,
                                                                  p_frame_y_q_scale)
        self.digest = FrameDigest(i_net.dev) if digest else None
        header_bit_depth(bit_depth)     # before the file is created
        self.schedule = KeyframeSchedule(gop_size, min_keyframe_interval)
        self.writer = SequenceWriter(path, self.codec, fmt, prec, width, height, bit_depth=bit_depth)
        self.dpb = None
        self.n = 0

    def encode(self, x, keyframe=False):
        frame_idx = self.n
        with torch.no_grad():
            if self.schedule.next(cut=bool(keyframe)) == "I":
                if self.codec == "DC":
                    out = self.i_net.encode_frame(x, self.q[0], self.q[1], self.height, self.width)
                else:
                    out = self.i_net.encode_frame(x, self.q[0], self.height, self.width)
                self.dpb = _i_dpb(self.codec, out["x_hat"])
                ftype = "I"
            else:
                if self.codec == "DC":
                    out = self.p_net.encode_frame(x, self.dpb, self.q[0], self.q[1], frame_idx % 4)
                else:
                    out = self.p_net.encode_frame(x, self.dpb, self.q[1], self.q[2])
                self.dpb = out["dpb"]
                ftype = "P"
            dig = self.digest(self.dpb) if self.digest is not None else None
        self.writer.write(ftype, out["payload"], twin=out["precision_fallback"] == "parity", digest=dig)
        self.n += 1
        return dict(out, type=ftype, recon=self.dpb["ref_frame"], digest=dig)

    def close(self):
        self.writer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class _FrameCount(int):
    """``SequenceDecoder.frames``: the file's frame count (an int, as it has
    always been), which can also be called: ``dec.frames(start, count)`` is the
    generator of those frames."""

    def __new__(cls, n, generator):
        self = super().__new__(cls, n)
        self._generator = generator
        return self

    def __call__(self, start=0, count=None):
        return self._generator(start, count)


class SequenceDecoder:
    """Decoder only: iterating yields, per frame, {"type", "x_hat" (the
    (1, 3, H, W) decoded frame), "dpb", "bit"}; ``frames(start, count)`` yields
    a range of them, decoding from the last keyframe before it (``frames`` is
    also the file's frame count).  Raises ValueError when the
    nets are not what the header says wrote the file, DigestMismatch when a
    stored digest is not the digest of this decoder's DPB, and
    SequenceFormatError on a truncated or unclosed file."""

    def __init__(self, i_net, p_net, path):
        mine = _describe(i_net, p_net)
        self.reader = SequenceReader(path)
        r = self.reader
        theirs = (r.codec, r.format, r.precision)
        if mine != theirs:
            r.close()
            raise ValueError(f"{path} was written by {theirs} codecs (codec, format, precision); these are {mine}")
        self.i_net, self.p_net, self.codec = i_net, p_net, r.codec
        self.width, self.height, self.frames = r.width, r.height, _FrameCount(r.frames, self._frames)
        self.digest = FrameDigest(i_net.dev)
        self.last_keyframe = self.frames_decoded = None     # set by frames()

    def __iter__(self):
        return self._decode(self.reader, 0)

    def _decode(self, records, first):
        """Decode ``records`` (frame ``first`` on), verifying every stored digest."""
        dpb = None
        for idx, rec in enumerate(records, first):
            with torch.no_grad():
                if rec["type"] == "I":
                    x_hat = self.i_net.decode_frame(rec["payload"], None, self.height, self.width,
                                                    fallback=rec["twin"])["x_hat"]
                    dpb = _i_dpb(self.codec, x_hat)
                else:
                    if dpb is None:
                        raise SequenceFormatError(f"{self.reader.path}: frame {idx} is a P frame with no frame before it")
                    dpb = self.p_net.decode_frame(rec["payload"], dpb, self.height, self.width,
                                                  fallback=rec["twin"])["dpb"]
                if rec["digest"] is not None:
                    got = self.digest(dpb)
                    if got != rec["digest"]:
                        raise DigestMismatch(idx, rec["digest"], got)
            yield {"type": rec["type"], "x_hat": dpb["ref_frame"], "dpb": dpb, "bit": len(rec["payload"]) * 8}

    def seek(self, start=0, count=None):
        """(keyframe entry, stop) of ``frames(start, count)``: the ``IndexEntry``
        of the last I frame at or before ``start`` and the index after the last
        frame it yields.  Reads record headers only; raises ValueError for a
        ``start`` outside the file or a ``count`` below 1."""
        from .lanes import keyframe_before
        if count is not None and (isinstance(count, bool) or not isinstance(count, int) or count < 1):
            raise ValueError(f"count {count!r} is not None or an integer >= 1")
        key = keyframe_before(self.reader.index(), start, self.reader.path)
        total = self.reader.frames
        return key, total if count is None else min(total, start + count)

    def _frames(self, start=0, count=None):
        """``frames(start, count)``: the frames ``start .. start + count - 1``
        (to the end of the file when ``count`` is None or reaches past it), as
        a generator; ``frames`` is this, callable.  Each frame is as ``__iter__`` yields
        it plus "frame_idx".  Decoding starts at the last keyframe at or before
        ``start`` (``lanes.keyframe_before``) and reads no payload before it;
        the frames between the keyframe and ``start`` are decoded, verified
        against their stored digests like the others, and dropped.
        ``last_keyframe`` and ``frames_decoded`` say afterwards where the call
        started and how many frames it decoded."""
        if self.reader.frames == 0 and start == 0 and count is None:
            return iter(())                     # a file of no frames, read from its start
        key, stop = self.seek(start, count)     # a bad range raises here, at the call
        return self._range(key, start, stop)

    def _range(self, key, start, stop):
        self.last_keyframe, self.frames_decoded = key.frame_idx, 0
        records = self.reader.records_from(key, stop - key.frame_idx)
        for idx, out in enumerate(self._decode(records, key.frame_idx), key.frame_idx):
            self.frames_decoded += 1
            if idx >= start:
                yield dict(out, frame_idx=idx)

    def close(self):
        self.reader.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ------------------------------------------------------------ command line
def _load_nets(a):
    from .layers import Precision
    from .stream_helper import get_state_dict
    if a.codec == "hem":
        from .hem import IntraNoAR, DMC
    else:
        from .dc import IntraNoAR, DMC
    prec = getattr(Precision, a.precision)()
    i_net = IntraNoAR(precision=prec).load_state_dict(get_state_dict(a.i_frame_model_path))
    p_net = DMC(precision=prec).load_state_dict(get_state_dict(a.p_frame_model_path))
    for net in (i_net, p_net):
        net.update(force=True)
        net.codec_format = FORMATS[int(a.yuv420)]
    return i_net, p_net


def main(argv=None):
    import argparse
    import json
    from . import harness
    ap = argparse.ArgumentParser(prog="python -m dcvc_amd.sequence", description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=("encode", "decode"))
    ap.add_argument("--codec", choices=("dc", "hem"), default="dc")
    ap.add_argument("--precision", choices=("split", "parity"), default="split")
    ap.add_argument("--i_frame_model_path", required=True)
    ap.add_argument("--p_frame_model_path", required=True)
    ap.add_argument("--yuv420", action="store_true", help="the checkpoints are YUV420 models (dist_in_yuv420)")
    ap.add_argument("--seq_path", required=True, help="the sequence file to write (encode) or read (decode)")
    ap.add_argument("--src_type", choices=("png", "yuv420", "yuv422", "yuv444", "rgb"), default=None,
                    help="png folder, raw planar .yuv (4:2:0, 4:2:2 or 4:4:4) or raw planar .rgb file; "
                         "decode: the layout of the decoded-frame files")
    ap.add_argument("--bit-depth", "--bit_depth", dest="bit_depth", type=int, default=None,
                    help="encode: bits per sample of a raw .yuv / .rgb source (8; 9..16: little-endian uint16); "
                         "decode: of the decoded-frame files (default: the source depth in the file's header)")
    ap.add_argument("--src_path")
    ap.add_argument("--src_width", type=int)
    ap.add_argument("--src_height", type=int)
    ap.add_argument("--frame_num", type=int,
                    help="encode: frames to code; decode: frames to emit (default: to the end)")
    ap.add_argument("--gop_size", type=int, default=32)
    ap.add_argument("--scene_cut", type=float, default=None,
                    help="encode: code a keyframe where the histogram distance hd of the source reaches this "
                         "threshold in (0, 1] (default: off; there is no default threshold)")
    ap.add_argument("--scene_cut_mad", type=float, default=None,
                    help="encode: the same on the mean absolute difference mad")
    ap.add_argument("--min_keyframe_interval", type=int, default=1,
                    help="encode: frames that must have passed since the last keyframe before a cut makes another")
    ap.add_argument("--start_frame", type=int, default=0,
                    help="decode: first frame to emit; decoding starts at the last keyframe at or before it")
    ap.add_argument("--q_in_ckpt", action="store_true")
    ap.add_argument("--q_index", type=int, default=None)
    ap.add_argument("--i_frame_q_scale", type=float, default=None)
    ap.add_argument("--p_frame_mv_y_q_scale", type=float, default=None)
    ap.add_argument("--p_frame_y_q_scale", type=float, default=None)
    ap.add_argument("--no_digest", action="store_true")
    ap.add_argument("--recon_path", default=None, help="decode: folder for the decoded frames")
    a = ap.parse_args(argv)
    i_net, p_net = _load_nets(a)
    args = {"seq_path": a.seq_path, "dist_in_yuv420": a.yuv420, "digest": not a.no_digest}
    if a.src_type is not None:
        args["src_type"] = a.src_type
    if a.bit_depth is not None:
        args["src_bit_depth" if a.mode == "encode" else "recon_bit_depth"] = a.bit_depth
    if a.mode == "encode":
        args.update(src_path=a.src_path, src_width=a.src_width, src_height=a.src_height, frame_num=a.frame_num,
                    gop_size=a.gop_size, q_in_ckpt=a.q_in_ckpt, i_frame_q_index=a.q_index,
                    i_frame_q_scale=a.i_frame_q_scale, p_frame_mv_y_q_scale=a.p_frame_mv_y_q_scale,
                    p_frame_y_q_scale=a.p_frame_y_q_scale, verbose=1, scene_cut=a.scene_cut,
                    scene_cut_mad=a.scene_cut_mad, min_keyframe_interval=a.min_keyframe_interval)
        out = harness.encode_video(i_net, p_net, args)
    else:
        args.update(start_frame=a.start_frame, frame_num=a.frame_num)
        if a.recon_path is not None:
            args.update(save_decoded_frame=True, recon_path=a.recon_path, decoded_frame_folder=a.recon_path)
        out = harness.decode_video(i_net, p_net, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The sequence file (dcvc_amd/sequence.py, INTEGRATION.md "Sequence file") on
the host: what is written comes back unchanged, damaged files raise the
documented error, and the bytes-level frame records are the reference-format
frame files."""
import struct

import pytest

from dcvc_amd.sequence import (SequenceWriter, SequenceReader, SequenceFormatError, MAGIC, NOT_CLOSED)

PAYLOADS = [b"", b"\x5a", bytes((i * 7 + i // 251) & 0xFF for i in range(70000))]
RECORDS = [("I", PAYLOADS[2], False, (0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF)),
           ("P", PAYLOADS[0], True, None),
           ("P", PAYLOADS[1], True, (0, 1 << 63)),
           ("P", PAYLOADS[1], False, None)]


def _write(path, records=RECORDS, close=True):
    w = SequenceWriter(path, "HEM", "yuv420", "split", 1920, 1080)
    for t, payload, twin, digest in records:
        w.write(t, payload, twin=twin, digest=digest)
    if close:
        w.close()
    else:
        w.file.flush()
    return w


def test_round_trip(tmp_path):
    p = str(tmp_path / "a.seq")
    _write(p)
    with SequenceReader(p) as r:
        assert (r.codec, r.format, r.precision, r.width, r.height, r.frames) == ("HEM", "yuv420", "split", 1920, 1080, 4)
        got = list(r)
    assert len(got) == len(RECORDS)
    for rec, (t, payload, twin, digest) in zip(got, RECORDS):
        assert rec == {"type": t, "twin": twin, "digest": digest, "payload": payload}


def test_layout_is_the_documented_one(tmp_path):
    """Byte by byte, as INTEGRATION.md lays it out (little endian)."""
    p = str(tmp_path / "a.seq")
    SequenceWriter(p, "DC", "rgb", "parity", 130, 100).close()
    head = open(p, "rb").read()
    assert len(head) == 40
    assert head[:8] == MAGIC == b"DCVCSEQ1"
    assert head[8] == 0 and head[9] == 0
    assert head[10:26] == b"parity" + b"\0" * 10
    assert head[26:28] == b"\0\0"
    assert struct.unpack("<III", head[28:40]) == (130, 100, 0)
    _write(p, RECORDS[1:3])
    data = open(p, "rb").read()
    assert data[8] == 1 and data[9] == 1 and struct.unpack("<I", data[36:40]) == (2,)
    r0 = data[40:64]
    assert r0 == bytes([1, 1, 0, 0]) + struct.pack("<IQQ", 0, 0, 0)
    r1 = data[64:88]
    assert r1 == bytes([1, 3, 0, 0]) + struct.pack("<IQQ", 1, 0, 1 << 63)
    assert data[88:] == PAYLOADS[1]


def test_unclosed_file(tmp_path):
    p = str(tmp_path / "a.seq")
    w = _write(p, close=False)
    assert struct.unpack("<I", open(p, "rb").read()[36:40]) == (NOT_CLOSED,)
    with pytest.raises(SequenceFormatError, match="not closed"):
        SequenceReader(p)
    w.close()
    assert SequenceReader(p).frames == 4


@pytest.mark.parametrize("cut", [40 + 24 + 100, 40 + 24 + 70000 + 10, 40 + 24 + 70000 + 24 + 24 + 1])
def test_truncated_file(tmp_path, cut):
    """Cut inside a payload, inside a record header, and between records."""
    p = str(tmp_path / "a.seq")
    _write(p)
    data = open(p, "rb").read()
    assert cut < len(data)
    open(p, "wb").write(data[:cut])
    with SequenceReader(p) as r, pytest.raises(SequenceFormatError, match="truncated"):
        list(r)


def test_wrong_magic(tmp_path):
    p = str(tmp_path / "a.seq")
    _write(p)
    data = open(p, "rb").read()
    open(p, "wb").write(b"DCVCSEQ2" + data[8:])
    with pytest.raises(SequenceFormatError, match="not a DCVCSEQ1"):
        SequenceReader(p)
    open(p, "wb").write(data[:20])
    with pytest.raises(SequenceFormatError):
        SequenceReader(p)
    assert issubclass(SequenceFormatError, ValueError)


def test_pack_functions_are_the_frame_files(tmp_path):
    """pack_i / pack_p are what encode_i / encode_p write, and unpack what
    decode_i / decode_p read, for DC and HEM."""
    from dcvc_amd import stream_helper as dc
    from dcvc_amd.hem import stream_helper as hem
    stream = bytes(range(256)) * 3
    p = str(tmp_path / "f.bin")
    dc.encode_i(1080, 1920, True, 63, stream, p)
    data = open(p, "rb").read()
    assert data == dc.pack_i(1080, 1920, True, 63, stream)
    assert dc.unpack_i(data) == dc.decode_i(p) == (1080, 1920, True, 63, stream)
    dc.encode_p(stream, False, 21, 3, p)
    data = open(p, "rb").read()
    assert data == dc.pack_p(stream, False, 21, 3)
    assert dc.unpack_p(data) == dc.decode_p(p) == (False, 21, 3, stream)
    hem.encode_i(100, 130, 154, stream, p)
    data = open(p, "rb").read()
    assert data == hem.pack_i(100, 130, 154, stream)
    assert hem.unpack_i(data) == hem.decode_i(p) == (100, 130, 154, stream)
    hem.encode_p(stream, 120, 65500, p)
    data = open(p, "rb").read()
    assert data == hem.pack_p(stream, 120, 65500)
    assert hem.unpack_p(data) == hem.decode_p(p) == (120, 65500, stream)

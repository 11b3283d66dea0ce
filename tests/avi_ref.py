"""A RIFF walker for the Motion-JPEG AVI 1.0 files of tokensgen_amd.jpeg.MJPEGWriter: it checks every size and nesting rule on the way and returns the headers,
the chunks and the index."""
import struct
from types import SimpleNamespace


def _chunks(buf, start, end):
    """the chunks (fourcc, payload start, size) that tile buf[start:end] exactly, each padded to an even length"""
    out, pos = [], start
    while pos < end:
        assert pos + 8 <= end, f"chunk header at {pos} crosses the end of its list at {end}"
        fourcc, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        assert pos + 8 + size <= end, f"chunk {fourcc!r} at {pos} ({size} bytes) crosses the end of its list at {end}"
        out.append((fourcc, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == end or pos == end + 1, f"chunks end at {pos}, their list at {end}"
    return out


def _list(buf, chunk, kind):
    fourcc, start, size = chunk
    assert fourcc == b"LIST" and buf[start:start + 4] == kind, f"expected LIST {kind!r}, found {fourcc!r} {buf[start:start + 4]!r}"
    return _chunks(buf, start + 4, start + size)


def walk(buf):
    """bytes of a whole file -> SimpleNamespace(avih, strh, strf: dicts; frames: list of bytes; index: list of (flags, offset, size); movi: offset of the fourcc)"""
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI ", "not a RIFF AVI file"
    riff = struct.unpack_from("<I", buf, 4)[0]
    assert riff + 8 == len(buf), f"RIFF size {riff} + 8 != file size {len(buf)}"
    assert len(buf) <= (1 << 31) - 1
    top = _chunks(buf, 12, len(buf))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"], [c[0] for c in top]
    hdrl = _list(buf, top[0], b"hdrl")
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56
    names = ("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams", "suggested_buffer", "width", "height")
    avih = dict(zip(names, struct.unpack_from("<10I", buf, hdrl[0][1])))
    strl = _list(buf, hdrl[1], b"strl")
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    p = strl[0][1]
    names = ("flags", "priority", "language", "initial_frames", "scale", "rate", "start", "length", "suggested_buffer", "quality", "sample_size")
    strh = dict(type=buf[p:p + 4], handler=buf[p + 4:p + 8], **dict(zip(names, struct.unpack_from("<IHHIIIIIIII", buf, p + 8))))
    strh["frame"] = struct.unpack_from("<4h", buf, p + 48)
    names = ("size", "width", "height", "planes", "bit_count", "compression", "size_image")
    strf = dict(zip(names, struct.unpack_from("<IiiHH4sI", buf, strl[1][1])))
    movi = top[1][1]
    chunks = _list(buf, top[1], b"movi")
    assert all(c[0] == b"00dc" for c in chunks)
    frames = [bytes(buf[s:s + n]) for _, s, n in chunks]
    assert top[2][2] % 16 == 0
    index = []
    for i in range(top[2][2] // 16):
        fourcc, flags, off, size = struct.unpack_from("<4sIII", buf, top[2][1] + 16 * i)
        assert fourcc == b"00dc"
        index.append((flags, off, size))
    # what the pieces say about each other
    assert len(index) == len(chunks) == avih["total_frames"] == strh["length"], (len(index), len(chunks), avih["total_frames"], strh["length"])
    for (flags, off, size), (_, s, n) in zip(index, chunks):
        assert flags == 0x10 and movi + off == s - 8 and size == n, "an index entry does not point at its chunk"
    assert avih["flags"] & 0x10 and avih["streams"] == 1
    assert strh["type"] == b"vids" and strh["handler"] == b"MJPG" and strf["compression"] == b"MJPG" and strf["size"] == 40 and strf["bit_count"] == 24 and strf["planes"] == 1
    assert (strf["width"], strf["height"]) == (avih["width"], avih["height"])
    largest = max((len(f) for f in frames), default=0)
    assert avih["suggested_buffer"] >= largest and strh["suggested_buffer"] >= largest
    return SimpleNamespace(avih=avih, strh=strh, strf=strf, frames=frames, index=index, movi=movi)

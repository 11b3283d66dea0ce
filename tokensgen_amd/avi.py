"""The Motion-JPEG AVI 1.0 container alone: RIFF bytes in and out, no tensor and no device.  `AVIWriter` takes frames that are JPEG streams
already and `AVIReader` hands them back; tokensgen_amd.jpeg puts the encoder and the decoder around them as MJPEGWriter and MJPEGReader, the names the messages
here carry.  Plain Python on the standard library alone, so the container can be read and tested without the codec; tests/avi_ref.py walks the files."""
import os
import struct
from fractions import Fraction

AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10
_MOVI_FOURCC = 220                              # RIFF 12, LIST hdrl 8 + 192, LIST movi 8: where the 'movi' fourcc stands; the first chunk follows at 224


class AVIWriter:
    """A Motion-JPEG AVI 1.0 file, written as the frames arrive: RIFF 'AVI ' { LIST 'hdrl' { avih, LIST 'strl' { strh vids/MJPG, strf BITMAPINFOHEADER } }, LIST 'movi'
    { 00dc chunks, padded to even length }, idx1 }.  `write_jpegs(chunks, height, width)` any number of times, then `close()`, which writes the index and the counts
    and sizes of the headers; or use it as a context manager.  All frames of a file have one size.  fps is any positive number:
    dwRate / dwScale = Fraction(fps).limit_denominator(65535).  A write that would take the file past MAX_FILE_BYTES (2^31 - 1: no OpenDML) is refused whole with
    a ValueError, and `close()` still leaves a valid file of the frames before it."""

    MAX_FILE_BYTES = (1 << 31) - 1

    def __init__(self, path, fps):
        if isinstance(fps, bool) or not isinstance(fps, (int, float, Fraction)) or not 0 < fps < float("inf"):
            raise ValueError(f"MJPEGWriter: fps must be a positive finite number, got {fps!r}")
        rate = Fraction(fps).limit_denominator(65535)
        if rate <= 0 or rate.numerator >= 1 << 32:
            raise ValueError(f"MJPEGWriter: fps {fps!r} has no dwRate / dwScale")
        self.path, self.rate = path, rate
        self.size = None                        # (H, W) of the first frame
        self._index = []                        # (offset from the 'movi' fourcc, bytes) per frame
        self._pos = _MOVI_FOURCC + 4            # file position == bytes so far
        self._fh = open(path, "wb")
        self._fh.write(b"\0" * self._pos)       # the headers are written by close(), when the counts are known

    @property
    def frames(self):
        return len(self._index)

    def _final_bytes(self, pos, n):
        return pos + 8 + 16 * n

    def check_size(self, H, W):
        if self.size is not None and self.size != (H, W):
            raise ValueError(f"MJPEGWriter: all frames of a file have one size; the file holds {self.size[0]} x {self.size[1]}, got {H} x {W}")

    def write_jpegs(self, chunks, height, width):
        """Frames that are JPEG streams already (a list of bytes, each of a height x width frame; what `jpeg_bytes` returns), appended in order."""
        if self._fh is None:
            raise ValueError("MJPEGWriter.write_jpegs: the file is closed")
        H, W = int(height), int(width)
        if not 1 <= H <= 65535 or not 1 <= W <= 65535 or any(not isinstance(c, (bytes, bytearray)) or c[:2] != b"\xff\xd8" or c[-2:] != b"\xff\xd9" for c in chunks):
            raise ValueError("MJPEGWriter.write_jpegs: expected JPEG streams (SOI .. EOI) of one height x width in 1..65535")
        self.check_size(H, W)
        pos = self._pos + sum(8 + len(c) + (len(c) & 1) for c in chunks)
        if self._final_bytes(pos, len(self._index) + len(chunks)) > self.MAX_FILE_BYTES:
            raise ValueError(f"MJPEGWriter: {len(chunks)} more frames would take {self.path} past {self.MAX_FILE_BYTES} bytes (AVI 1.0, no OpenDML); "
                             f"the file keeps its {len(self._index)} frames")
        self.size = (H, W)
        for c in chunks:
            self._index.append((self._pos - _MOVI_FOURCC, len(c)))
            self._fh.write(b"00dc" + struct.pack("<I", len(c)) + bytes(c) + b"\0" * (len(c) & 1))
            self._pos += 8 + len(c) + (len(c) & 1)
        return len(chunks)

    def close(self):
        if self._fh is None:
            return
        fh, self._fh = self._fh, None
        n, (H, W) = len(self._index), self.size or (0, 0)
        largest = max((s for _, s in self._index), default=0)
        fh.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, o, s) for o, s in self._index))
        total = self._final_bytes(self._pos, n)
        rate, scale = self.rate.numerator, self.rate.denominator
        avih = struct.pack("<14I", round(1e6 * scale / rate), min(int(largest * rate / scale) + 1, 0xffffffff) if n else 0, 0, AVIF_HASINDEX, n, 0, 1, largest, W, H,
                           0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, scale, rate, 0, n, largest, 0xffffffff, 0, 0, 0, min(W, 32767),
                                        min(H, 32767))
        strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", min(3 * W * H, 0xffffffff), 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + \
            struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", self._pos - _MOVI_FOURCC) + b"movi"
        assert len(head) == _MOVI_FOURCC + 4
        fh.seek(0)
        fh.write(head)
        fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class AVIReader:
    """A Motion-JPEG AVI 1.0 file (ours, or any baseline MJPG AVI): `.frames` / len(), `.size` (H, W) of the stream header, `.fps` (a Fraction, dwRate / dwScale),
    `get_avg_fps()`; `frame_bytes(indices)` returns the frames' JPEG streams; an index may repeat.
    The first `strl` whose `strh` is `vids` with handler or biCompression MJPG is the stream; its NNdc / NNdb chunks are the frames, other streams' chunks are skipped,
    LIST 'rec ' is walked.  `idx1` is used when present (offsets relative to the 'movi' fourcc or to the file: whichever finds the chunk's fourcc), otherwise `movi` is
    walked.  A chunk of length 0 repeats the frame before it.  OpenDML (RIFF AVIX, indx) and other codecs are refused by name; a truncated file is a ValueError.  The
    constructor reads the headers and the index only; the frames are read from the file when asked for.  A context manager."""

    def __init__(self, path):
        self.path = path
        self._fh = open(path, "rb")
        try:
            self._parse()
        except BaseException:
            self.close()
            raise

    def _bad(self, what):
        return ValueError(f"MJPEGReader: {self.path}: {what}")

    def _read_at(self, pos, n, what):
        if pos < 0 or pos + n > self._size:
            raise self._bad(f"the file is truncated: {what} at byte {pos} needs {n} bytes, the file has {self._size}")
        self._fh.seek(pos)
        return self._fh.read(n)

    def _parse(self):
        path, read_at = self.path, self._read_at
        self._fh.seek(0, os.SEEK_END)
        size = self._size = self._fh.tell()
        head = read_at(0, 12, "the RIFF header")
        if head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise self._bad("not a RIFF 'AVI ' file")
        riff_end = 8 + struct.unpack_from("<I", head, 4)[0]
        if riff_end > size:
            raise self._bad(f"the file is truncated: RIFF says {riff_end} bytes, the file has {size}")
        after = riff_end + (riff_end & 1)
        if after + 12 <= size and read_at(after, 12, "a second RIFF")[8:12] == b"AVIX":
            raise NotImplementedError(f"MJPEGReader: {path}: OpenDML (a RIFF 'AVIX' extension); AVI 1.0 only")
        stream, rate, scale, dims, movi, idx1 = None, None, None, None, None, None
        pos = 12
        while pos + 8 <= riff_end:
            fourcc, n = struct.unpack("<4sI", read_at(pos, 8, "a chunk header"))
            if pos + 8 + n > riff_end:
                raise self._bad(f"the file is truncated: chunk {fourcc!r} at byte {pos} ({n} bytes) runs past the end at {riff_end}")
            if fourcc == b"LIST":
                kind = read_at(pos + 8, 4, "a LIST type")
                if kind == b"hdrl":
                    stream, rate, scale, dims = self._parse_hdrl(read_at(pos + 12, n - 4, "the header list"))
                elif kind == b"movi":
                    movi = (pos + 8, pos + 8 + n)                               # from the 'movi' fourcc to the end of the list
            elif fourcc == b"idx1":
                idx1 = (pos + 8, n)
            pos += 8 + n + (n & 1)
        if stream is None:
            raise NotImplementedError(f"MJPEGReader: {path}: no video stream with codec MJPG (handler or biCompression); Motion-JPEG only")
        if movi is None:
            raise self._bad("no LIST 'movi'")
        tags = (b"%02ddc" % stream, b"%02ddb" % stream)
        entries = []                                                            # (payload position, bytes)
        if idx1 is not None and idx1[1] >= 16:
            raw = read_at(idx1[0], idx1[1] - idx1[1] % 16, "idx1")
            rows = [struct.unpack_from("<4sIII", raw, i) for i in range(0, len(raw), 16)]
            ours = [r for r in rows if r[0] in tags]
            base = None
            if ours:
                for cand in (movi[0], 0):                                       # relative to the 'movi' fourcc, or to the file
                    p = cand + ours[0][2]
                    if 0 <= p and p + 8 <= size and read_at(p, 4, "an indexed chunk") == ours[0][0]:
                        base = cand
                        break
                if base is None:
                    raise self._bad("idx1 does not point at the first frame's chunk, from the 'movi' list or from the file start")
            for fourcc, _, off, n in ours:
                if base + off + 8 + n > size:
                    raise self._bad(f"the file is truncated: an indexed frame at byte {base + off} ({n} bytes) runs past the end at {size}")
                entries.append((base + off + 8, n))
        else:
            self._walk(movi[0] + 4, movi[1], tags, entries)
        self._entries = []
        for p, n in entries:
            if n == 0:
                if not self._entries:
                    raise self._bad("the first frame is a zero-length chunk: there is no frame before it to repeat")
                self._entries.append(self._entries[-1])
            else:
                self._entries.append((p, n))
        self.fps = Fraction(rate, scale)
        self.size = dims

    @staticmethod
    def _parse_hdrl(buf):
        """-> (stream number, dwRate, dwScale, (H, W)) of the first MJPG video stream, or (None, ..)"""
        pos, number = 0, 0
        while pos + 8 <= len(buf):
            fourcc, n = struct.unpack_from("<4sI", buf, pos)
            if fourcc == b"LIST" and buf[pos + 8:pos + 12] == b"strl":
                strh = strf = None
                has_indx = False
                q, end = pos + 12, min(pos + 8 + n, len(buf))
                while q + 8 <= end:
                    cc, m = struct.unpack_from("<4sI", buf, q)
                    if cc == b"strh":
                        strh = buf[q + 8:q + 8 + m]
                    elif cc == b"strf":
                        strf = buf[q + 8:q + 8 + m]
                    elif cc == b"indx":
                        has_indx = True
                    q += 8 + m + (m & 1)
                if strh is not None and len(strh) >= 28 and strh[:4] == b"vids":
                    codec = strf[16:20] if strf is not None and len(strf) >= 20 else b""
                    if strh[4:8].upper() == b"MJPG" or codec.upper() == b"MJPG":
                        if has_indx:
                            raise NotImplementedError("MJPEGReader: OpenDML (an 'indx' super index in the stream header); AVI 1.0 only")
                        scale, rate = struct.unpack_from("<II", strh, 20)
                        if scale < 1 or rate < 1:
                            raise ValueError(f"MJPEGReader: the stream header has no frame rate (dwRate {rate} / dwScale {scale})")
                        dims = struct.unpack_from("<ii", strf, 4) if strf is not None and len(strf) >= 12 else (0, 0)
                        return number, rate, scale, (abs(dims[1]), dims[0])
                    raise NotImplementedError(f"MJPEGReader: video codec {strh[4:8]!r} / {codec!r}; Motion-JPEG (MJPG) only")
                number += 1
            pos += 8 + n + (n & 1)
        return None, None, None, None

    def _walk(self, pos, end, tags, entries):
        while pos + 8 <= end:
            fourcc, n = struct.unpack("<4sI", self._read_at(pos, 8, "a chunk header"))
            if pos + 8 + n > end:
                raise self._bad(f"the file is truncated: chunk {fourcc!r} at byte {pos} ({n} bytes) runs past the end of 'movi' at {end}")
            if fourcc == b"LIST":
                if self._read_at(pos + 8, 4, "a LIST type") == b"rec ":
                    self._walk(pos + 12, pos + 8 + n, tags, entries)
            elif fourcc in tags:
                entries.append((pos + 8, n))
            elif fourcc[:2] == b"ix":
                raise NotImplementedError(f"MJPEGReader: {self.path}: OpenDML (an '{fourcc.decode('latin1')}' index chunk); AVI 1.0 only")
            pos += 8 + n + (n & 1)

    @property
    def frames(self):
        return len(self._entries)

    def __len__(self):
        return len(self._entries)

    def get_avg_fps(self):
        return float(self.fps)

    def frame_bytes(self, indices):
        """the JPEG streams of those frames, from the file"""
        if self._fh is None:
            raise ValueError("MJPEGReader: the file is closed")
        out, cache = [], {}
        for i in indices:
            i = int(i)
            if not -len(self) <= i < len(self):
                raise IndexError(f"MJPEGReader: frame {i} of {len(self)}")
            p, n = self._entries[i]
            if p not in cache:
                self._fh.seek(p)
                cache[p] = self._fh.read(n)
                if len(cache[p]) != n:
                    raise self._bad(f"the file is truncated: frame {i} at byte {p} has {len(cache[p])} of {n} bytes")
            out.append(cache[p])
        return out

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

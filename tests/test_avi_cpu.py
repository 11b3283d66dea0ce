"""tokensgen_amd.avi, the Motion-JPEG AVI 1.0 container alone: no tensor library behind it, and a round trip of hand-made streams through its two classes, held to
the RIFF walker of tests/avi_ref.py.  The codec around it (tokensgen_amd.jpeg) has its own tests."""
import os
import struct
import subprocess
import sys
from fractions import Fraction

import pytest

import avi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_container_imports_no_tensor_library():
    code = ("import sys; sys.path.insert(0, %r); import tokensgen_amd.avi as avi\n"
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules and 'tokensgen_amd.kernels' not in sys.modules, sorted(m for m in sys.modules if '.' not in m)\n"
            "assert avi.AVIWriter.MAX_FILE_BYTES == 2 ** 31 - 1") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_round_trip_of_hand_made_streams(tmp_path):
    from tokensgen_amd import avi
    odd, even = b"\xff\xd8" + bytes(range(1, 6)) + b"\xff\xd9", b"\xff\xd8" + bytes(range(10, 16)) + b"\xff\xd9"     # 9 bytes (one pad byte) and 10
    assert len(odd) & 1 and not len(even) & 1
    path = tmp_path / "a.avi"
    with avi.AVIWriter(path, Fraction(30000, 1001)) as w:
        assert w.write_jpegs([odd], 6, 10) == 1 and w.write_jpegs([even], 6, 10) == 1 and w.frames == 2 and w.size == (6, 10)
        with pytest.raises(ValueError, match="MJPEGWriter: all frames of a file have one size"):
            w.write_jpegs([odd], 6, 12)
        with pytest.raises(ValueError, match="MJPEGWriter.write_jpegs: expected JPEG streams"):
            w.write_jpegs([odd[:-1]], 6, 10)
    raw = path.read_bytes()
    a = avi_ref.walk(raw)
    assert a.frames == [odd, even] and a.movi == 220 and [(off, n) for _, off, n in a.index] == [(4, 9), (4 + 8 + 10, 10)]      # the pad byte is between them
    assert len(raw) == 224 + (8 + 10) + (8 + 10) + 8 + 2 * 16
    assert (a.avih["width"], a.avih["height"], a.strh["rate"], a.strh["scale"]) == (10, 6, 30000, 1001)
    with avi.AVIReader(path) as r:
        assert len(r) == r.frames == 2 and r.size == (6, 10) and r.fps == Fraction(30000, 1001)
        assert r.frame_bytes([0, 1, -1, 0]) == [odd, even, even, odd]
    with pytest.raises(ValueError, match="MJPEGReader: the file is closed"):
        r.frame_bytes([0])
    # a zero-length chunk repeats the frame before it: spliced in behind the odd frame and its pad byte, the index dropped so that 'movi' is walked
    movi = raw[224:224 + 18] + b"00dc" + struct.pack("<I", 0) + raw[224 + 18:224 + 36]
    spliced = raw[:216] + struct.pack("<I", 4 + len(movi)) + b"movi" + movi
    spliced = spliced[:4] + struct.pack("<I", len(spliced) - 8) + spliced[8:]
    (tmp_path / "z.avi").write_bytes(spliced)
    with avi.AVIReader(tmp_path / "z.avi") as r:
        assert len(r) == 3 and r.frame_bytes(range(3)) == [odd, odd, even]
    (tmp_path / "t.avi").write_bytes(raw[:230])
    with pytest.raises(ValueError, match="MJPEGReader: .*truncated"):
        avi.AVIReader(tmp_path / "t.avi")

"""CPU: the reasoning behind the second pass of the segmented PNG path, with zlib as the inflate and the encoder's
restatement as the writer. A segment of this library's files may copy from the last four bytes of the segment before. Inflated with
two different leads, an output byte either agrees (its value is final) or is j / 255 - j (it is lead byte j); following those
references back through the segments gives every segment its true history, and the stream is the serial decoder's."""
import zlib

import numpy as np
import png_restatement as R
from dad_3dheads_amd import _lib

S, LEAD = _lib.PNG_SEGMENT_BYTES, 4
FIRST, SECOND = bytes([0, 1, 2, 3]), bytes([255, 254, 253, 252])


def inflate(payload, lead=b""):
    return (zlib.decompressobj(-15, zdict=lead) if lead else zlib.decompressobj(-15)).decompress(payload)


def two_passes(segments):
    """(stream, number of segments that needed their lead, longest walk back)"""
    out, tails, dependent = [], [], []
    for k, p in enumerate(segments):
        try:
            o, refs = inflate(p), [None] * LEAD
            dependent.append(False)
        except zlib.error:
            assert k > 0
            o, other = inflate(p, FIRST), inflate(p, SECOND)  # zlib refuses a distance past the four bytes
            assert len(o) == len(other)
            refs = []
            for x, y in zip(o[-LEAD:], other[-LEAD:]):
                assert x == y or (x < LEAD and y == 255 - x)
                refs.append(None if x == y else x)
            dependent.append(True)
        out.append(o)
        tails.append((o[-LEAD:], refs))
    longest = 0
    for k in range(1, len(segments)):
        if dependent[k]:
            history = []
            for j in range(LEAD):
                m, at = k - 1, j
                while tails[m][1][at] is not None:
                    at, m = tails[m][1][at], m - 1
                longest = max(longest, k - 1 - m)
                history.append(tails[m][0][at])
            out[k] = inflate(segments[k], bytes(history))
    return b"".join(out), sum(dependent), longest


def test_own_files_come_back_from_two_passes():
    needed = {}
    for name, img in R.fixture_images().items():
        info = R.read_png(R.png_file(img, S)[0])
        stream, needed[name], _ = two_passes(info["idat"][1:-1])
        assert stream == info["stream"], name
    assert any(needed.values()) and not all(needed.values())  # both kinds of file are among the fixtures


def test_a_run_through_every_segment_walks_back_to_the_first():
    img = np.zeros((40, 1023, 3), dtype=np.uint8)
    info = R.read_png(R.png_file(img, S)[0])
    segments = info["idat"][1:-1]
    stream, needed, longest = two_passes(segments)
    assert stream == info["stream"] and needed == len(segments) - 1 and longest == len(segments) - 2

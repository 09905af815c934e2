"""CPU: the JPEG decode rules held to PIL, twice: tests/jpeg_restatement.py, and dad3d_jpeg_decode_host, which runs
the `__host__ __device__` routines of csrc/jpeg_entropy.hpp and csrc/jpeg_idct.hpp that the kernels of csrc/jpeg_decode.hip run.
Bit-equal to `np.asarray(Image.open(f))` on a corpus PIL writes here and on the demo image (a foreign encoder's file) with no file
flagged; files outside the decoder and header defects each held to their flag; truncated and bit-flipped files held to "a flag, or
exactly PIL's pixels", and a file PIL refuses must be flagged."""
import numpy as np
import pytest

import jpeg_restatement as R
from jpeg_cases import MALFORMED, UNSUPPORTED, corpus, demo_bytes, header_defects, host_decode, jpeg, pil_array, pil_raises, picture, refused
from dad_3dheads_amd import jpeg_reader


def test_flags_mirror_the_restatement():
    assert (R.MALFORMED, R.UNSUPPORTED) == (MALFORMED, UNSUPPORTED)


def test_corpus_is_what_the_issue_asks():
    names = [n for n, _ in corpus()]
    assert len(names) >= 300 and len(set(names)) == len(names)
    assert all(pil_array(f).shape[0] <= 140 and pil_array(f).shape[1] <= 140 for _, f in corpus())
    assert any(b"\xff\xdd" in f for _, f in corpus())  # DRI


def test_host_entry_equals_pil_on_the_corpus_and_flags_nothing():
    flagged = []
    for name, f in corpus():
        flag, got = host_decode(f)
        if flag:
            flagged.append(name)
            continue
        assert np.array_equal(got, pil_array(f)), name
    assert flagged == []  # the share of flagged files is 0


def test_restatement_equals_pil_on_the_corpus_and_flags_nothing():
    flagged = []
    for name, f in corpus():
        flag, got = R.decode(f)
        if flag:
            flagged.append(name)
            continue
        assert np.array_equal(got, pil_array(f)), name
    assert flagged == []


def test_channel_conversion_equals_pils_convert():
    for name, f in corpus()[::7]:
        for channels in (1, 3):
            want = pil_array(f, channels)
            flag, got = host_decode(f, channels)
            assert flag == 0 and np.array_equal(got, want), (name, channels)
            flag, got = R.decode(f, channels)
            assert flag == 0 and np.array_equal(got, want), (name, channels)


def test_demo_image_of_a_foreign_encoder():
    f = demo_bytes()
    want = pil_array(f)
    assert want.shape == (954, 766, 3)
    flag, got = host_decode(f)
    assert flag == 0 and np.array_equal(got, want)
    flag, got = host_decode(f, 1)
    assert flag == 0 and np.array_equal(got, pil_array(f, 1))
    flag, got = R.decode(f)
    assert flag == 0 and np.array_equal(got, want)


def test_host_sizing_reads_up_to_sof_only():
    for name, f in corpus()[::11]:
        assert jpeg_reader._header(f) == pil_array(f).shape, name
    f = demo_bytes()
    assert jpeg_reader._header(f) == (954, 766, 3)
    sof = f.index(b"\xff\xc0")
    assert jpeg_reader._header_of(f[:sof + 10], len(f)) == (954, 766, 3) and jpeg_reader._header_of(f[:sof + 9], len(f)) is None
    assert jpeg_reader._header(b"") is None and jpeg_reader._header(b"\x89PNG\r\n\x1a\n" + bytes(40)) is None
    assert jpeg_reader._header(refused()["progressive"][0]) is None  # SOF2: PIL gets the file as it is
    assert jpeg_reader._header(refused()["CMYK"][0]) is None


@pytest.mark.parametrize("name", sorted(refused()))
def test_files_outside_the_decoder_are_flagged(name):
    f, flag = refused()[name]
    assert not pil_raises(f)
    assert host_decode(f)[0] == flag and R.decode(f)[0] == flag


@pytest.mark.parametrize("name", sorted(header_defects()))
def test_header_defects_are_flagged(name):
    f, flag = header_defects()[name]
    assert host_decode(f)[0] == flag, name
    assert R.decode(f)[0] == flag, name


def _flag_or_pils_pixels(f, what):
    flag, got = host_decode(f)
    if flag:
        assert got is None
        return True
    assert not pil_raises(f), what  # a file PIL refuses must be flagged
    assert np.array_equal(got, pil_array(f)), what
    return False


def test_truncated_files():
    small = [jpeg(picture((8, 8, 3), 1), quality=90), jpeg(picture((17, 9, 3), 2), quality=75, subsampling=2, restart_marker_blocks=1),
             jpeg(picture((12, 20), 3), quality=50)]
    for k, f in enumerate([demo_bytes()[:4096]] + small):
        assert k == 0 or _flag_or_pils_pixels(f, (k, "whole")) is False
        for n in range(len(f)):
            assert _flag_or_pils_pixels(f[:n], (k, n)), (k, n)  # no EOI: always a flag


def test_every_single_bit_flip_of_a_small_file():
    f = jpeg(picture((8, 8, 3), 4), quality=90)
    flagged = 0
    for at in range(len(f)):
        for bit in range(8):
            flagged += _flag_or_pils_pixels(f[:at] + bytes([f[at] ^ (1 << bit)]) + f[at + 1:], (at, bit))
    assert 0 < flagged < 8 * len(f)  # both ends of "a flag, or PIL's pixels" were met

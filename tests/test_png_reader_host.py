"""CPU: the host side of png_reader for the files the device does not take (`_pil_decode`). With `channels=None` nothing may be
lost silently: a palette file comes back as RGB, or RGBA where it has a tRNS chunk, a bilevel file as L, and a 16-bit file, whose
values `convert` would clamp to 255, is refused; with a channel count the pixels are PIL's `convert`."""
import io

import numpy as np
import pytest
from PIL import Image

from dad_3dheads_amd import png_reader


def saved(im, **kw):
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    return buf.getvalue()


def test_palette_and_bilevel_files_keep_their_content():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    palette = saved(Image.fromarray(rgb, "RGB").quantize(16))
    clear = saved(Image.fromarray(rgb, "RGB").quantize(16), transparency=2)
    bilevel = saved(Image.fromarray(rng.integers(0, 2, (6, 7), dtype=np.uint8) * 255, "L").convert("1"))
    assert Image.open(io.BytesIO(palette)).mode == "P" and "transparency" in Image.open(io.BytesIO(clear)).info
    for data, mode, c in ((palette, "RGB", 3), (clear, "RGBA", 4), (bilevel, "L", 1)):
        got = png_reader._pil_decode(data, None)
        want = np.asarray(Image.open(io.BytesIO(data)).convert(mode)).reshape(6, 7, c)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    alpha = png_reader._pil_decode(clear, None)[:, :, 3]
    assert (alpha == 0).any() and (alpha == 255).any()  # the tRNS entry arrived


def test_sixteen_bit_files_are_refused_without_a_channel_count():
    deep = np.random.default_rng(4).integers(256, 65536, (6, 7), dtype=np.uint16)
    data = saved(Image.fromarray(deep))
    assert data[24] == 16
    with pytest.raises(ValueError, match="uint8"):
        png_reader._pil_decode(data, None)
    for channels, mode in ((1, "L"), (3, "RGB")):  # asked for, the conversion is PIL's
        want = np.asarray(Image.open(io.BytesIO(data)).convert(mode)).reshape(6, 7, channels)
        assert np.array_equal(png_reader._pil_decode(data, channels), want)

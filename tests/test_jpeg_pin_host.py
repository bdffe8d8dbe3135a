"""The JPEG-domain front end on the host against libjpeg itself.  tests/golden/jpeg_golden.npz (tools/make_jpeg_goldens.py) holds small
images, the baseline JPEG files Pillow's libjpeg-turbo wrote for them at quality 100 (quantisation tables of ones) and the quantised
coefficients in those files, read back by tests/jpeg_coef_ref.py -- what the reference gets from TurboJPEG.encode + jpeg2dct.loads.
frontend.transform_dct_jpeg (colour conversion, 4:2:0 down-sampler, islow DCT, quantiser) and frontend.jpeg_quantised_dct must equal
them, every coefficient.  Only the two tests that call Pillow need it; the rest run from the npz."""
import io
import os

import numpy as np
import pytest

import jpeg_coef_ref as J

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "jpeg_golden.npz"))
RGB = [str(n) for n in G["rgb_names"]]
GRAY = [str(n) for n in G["gray_names"]]
BUILT_WITH = "fixtures written by Pillow %s / %s" % (G["pillow_version"], G["libjpeg_turbo_version"])


def _blocks_to_plane(coef):
    by, bx = coef.shape[:2]
    return coef.reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _block_sums(plane):
    """sum of (pixel - 128) per 8 x 8 block: eight times the exact DC term, so +-4 is a DC term of exactly +-0.5"""
    h, w = plane.shape
    return (plane.astype(np.int64) - 128).reshape(h // 8, 8, w // 8, 8).sum((1, 3))


# ------------------------------------------------------------------------------------------ the decoder and the fixtures
def test_fixture_inventory():
    assert 6 <= len(RGB) <= 8 and 3 <= len(GRAY) <= 4
    shapes = [G[f"rgb_{n}_img"].shape for n in RGB]
    assert all(s[0] % 16 == 0 and s[1] % 16 == 0 and max(s[:2]) <= 64 and s[2] == 3 for s in shapes)
    assert any(s[0] != s[1] for s in shapes)
    assert all(G[f"gray_{n}_plane"].ndim == 2 and G[f"gray_{n}_plane"].dtype == np.uint8 for n in GRAY)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "jpeg_golden.npz")) < 100 * 1024
    assert str(G["pillow_version"]) and str(G["libjpeg_turbo_version"])


@pytest.mark.parametrize("name", RGB)
def test_decoder_reproduces_colour_goldens(name):
    comps = J.decode_coefficients(G[f"rgb_{name}_jpeg"].tobytes())
    h, w = G[f"rgb_{name}_img"].shape[:2]
    assert [(c.h, c.v) for c in comps] == [(2, 2), (1, 1), (1, 1)]                          # 4:2:0
    assert [c.coef.shape for c in comps] == [(h // 8, w // 8, 64), (h // 16, w // 16, 64), (h // 16, w // 16, 64)]
    for tag, c in zip(("y", "cb", "cr"), comps):
        assert (c.qtable == 1).all(), "quality 100: the file's coefficients are the quantised ones"
        assert c.coef.dtype == G[f"rgb_{name}_{tag}"].dtype == np.int16 and np.array_equal(c.coef, G[f"rgb_{name}_{tag}"])


@pytest.mark.parametrize("name", GRAY)
def test_decoder_reproduces_gray_goldens(name):
    (c,) = J.decode_coefficients(G[f"gray_{name}_jpeg"].tobytes())
    h, w = G[f"gray_{name}_plane"].shape
    assert (c.qtable == 1).all() and c.coef.shape == (h // 8, w // 8, 64)
    assert np.array_equal(c.coef, G[f"gray_{name}_coef"])


def test_decoder_refuses_what_it_does_not_read():
    data = G[f"gray_{GRAY[0]}_jpeg"].tobytes()
    sof = data.index(b"\xff\xc0")
    with pytest.raises(J.JpegError, match="not baseline"):
        J.decode_coefficients(data[:sof] + b"\xff\xc2" + data[sof + 2:])                  # a progressive frame header
    sos = data.index(b"\xff\xda")
    with pytest.raises(J.JpegError, match="restart"):
        J.decode_coefficients(data[:sos] + b"\xff\xdd\x00\x04\x00\x08" + data[sos:])      # DRI, interval 8
    with pytest.raises(J.JpegError):
        J.decode_coefficients(data[:-40])                                                 # cut short
    with pytest.raises(J.JpegError, match="SOI"):
        J.decode_coefficients(data[2:])


@pytest.mark.parametrize("name", GRAY)
def test_decoder_against_pillow_decode(name):
    """an independent witness that the decoder reads the file right: the float inverse DCT of ITS coefficients is the image libjpeg
    decodes from the same bytes.  libjpeg's integer inverse DCT (jidctint) is good to under one grey level before its own rounding
    to uint8; the bound is that 1 level (0.57 measured when the fixtures were made)."""
    Image = pytest.importorskip("PIL.Image")
    from scipy.fft import idctn
    data = G[f"gray_{name}_jpeg"].tobytes()
    (c,) = J.decode_coefficients(data)
    by, bx = c.coef.shape[:2]
    blocks = c.coef.reshape(by, bx, 8, 8).astype(np.float64) * c.qtable.reshape(8, 8)
    rec = np.clip(idctn(blocks, axes=(2, 3), norm="ortho") + 128.0, 0.0, 255.0).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)
    pil = np.asarray(Image.open(io.BytesIO(data)))
    assert pil.shape == rec.shape and pil.dtype == np.uint8
    err = np.abs(pil.astype(np.float64) - rec).max()
    print(f"{name}: |Pillow decode - float IDCT of decoded coefficients| max = {err:.3f}")
    assert err <= 1.0


def test_regeneration_with_this_pillow():
    """re-encoding the committed images with the Pillow that is here gives the committed coefficients; a libjpeg build that writes
    other coefficients is reported with both version strings"""
    Image = pytest.importorskip("PIL.Image")
    import PIL
    from PIL import features
    here = "Pillow %s / libjpeg-turbo %s" % (PIL.__version__, features.version_feature("libjpeg_turbo") if features.check_feature("libjpeg_turbo") else None)

    def encode(arr, **kw):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(arr)).save(buf, "JPEG", quality=100, **kw)
        return J.decode_coefficients(buf.getvalue())

    for name in RGB:
        comps = encode(G[f"rgb_{name}_img"][..., ::-1], subsampling=2)
        for tag, c in zip(("y", "cb", "cr"), comps):
            assert (c.qtable == 1).all() and np.array_equal(c.coef, G[f"rgb_{name}_{tag}"]), f"{name}/{tag}: {here} disagrees with the {BUILT_WITH}"
    for name in GRAY:
        (c,) = encode(G[f"gray_{name}_plane"])
        assert (c.qtable == 1).all() and np.array_equal(c.coef, G[f"gray_{name}_coef"]), f"{name}: {here} disagrees with the {BUILT_WITH}"


# ------------------------------------------------------------------------------------------ the host paths, exactly
@pytest.mark.parametrize("name", RGB)
def test_transform_dct_jpeg_equals_libjpeg(name):
    from dctfhe import frontend
    got = frontend.transform_dct_jpeg(G[f"rgb_{name}_img"])
    for tag, g in zip(("y", "cb", "cr"), got):
        want = G[f"rgb_{name}_{tag}"]
        assert g.shape == want.shape and np.array_equal(g, want), f"{name}/{tag}: {int((g != want).sum())} of {want.size} coefficients differ"


@pytest.mark.parametrize("name", GRAY)
def test_jpeg_quantised_dct_equals_libjpeg(name):
    from dctfhe import frontend
    got = frontend.jpeg_quantised_dct(G[f"gray_{name}_plane"])
    want = G[f"gray_{name}_coef"]
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} coefficients differ"


# ------------------------------------------------------------------------------------------ what the fixtures cover (goldens only)
def test_fixtures_hold_dc_ties_of_both_signs():
    """the DC term of libjpeg's DCT is the exact block sum of (pixel - 128) (eight times the orthonormal DC), so a block sum of +-4
    is a quantiser input exactly on +-0.5, and libjpeg's answer (in the goldens) is +-1: half away from zero.  Luma planes of grey
    (R = G = B) images equal the grey value, so the colour fixture `dc_ties` is read the same way."""
    planes = [(G[f"gray_{n}_plane"], G[f"gray_{n}_coef"]) for n in GRAY]
    img = G["rgb_dc_ties_img"]
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all()
    planes.append((img[..., 0], G["rgb_dc_ties_y"]))
    up = down = 0
    for plane, coef in planes:
        s, dc = _block_sums(plane), coef[..., 0].astype(np.int64)
        assert np.array_equal(dc, np.where(s < 0, -((-s + 4) >> 3), (s + 4) >> 3))        # the golden DC terms are the rounded sums, ties away
        up += int(((s == 4) & (dc == 1)).sum())
        down += int(((s == -4) & (dc == -1)).sum())
        assert not ((s == 4) & (dc != 1)).any() and not ((s == -4) & (dc != -1)).any()
    assert up >= 2 and down >= 2, (up, down)
    # other ties (x.5 with x != 0) are there too: +-12 -> +-2, +-20 -> +-3
    s, dc = _block_sums(G["rgb_dc_ties_img"][..., 0]), G["rgb_dc_ties_y"][..., 0]
    assert set(zip(s.ravel().tolist(), dc.ravel().tolist())) >= {(12, 2), (-12, -2), (20, 3), (-20, -3)}


def test_fixtures_hold_saturated_coefficients():
    big = sum(int((np.abs(G[f"gray_{n}_coef"].astype(np.int64)) >= 1016).sum()) for n in GRAY)
    big += sum(int((np.abs(G[f"rgb_{n}_{t}"].astype(np.int64)) >= 1016).sum()) for n in RGB for t in ("y", "cb", "cr"))
    assert big >= 2
    sat = G["gray_saturated_coef"]
    assert sat.min() == -1024 and sat[..., 0].max() == 1016                               # all-0 and all-255 blocks
    assert np.abs(sat[..., 1:].astype(np.int64)).max() >= 900                             # and AC terms near the range's end


def test_fixtures_hit_both_phases_of_the_downsampler_bias():
    """libjpeg's 2x2 chroma average adds 1 at even output columns and 2 at odd ones before >> 2; only a 2x2 sum = 2 (mod 4) tells the
    two apart, sums = 1 and 3 fix the rounding direction either way.  The fixture `chroma_bias` has every class at both column
    parities, in Cb and in Cr.  The full-resolution chroma is computed here from the JFIF definition in float64; the fixture's pixels
    sit at least 0.1 from a rounding boundary, so any correct rounding of that definition gives the same integers."""
    bgr = G["rgb_chroma_bias_img"][..., ::-1].astype(np.float64)                          # what the encoder is handed
    r, g, b = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    for chroma in (128.0 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128.0 + 0.5 * r - 0.418688 * g - 0.081312 * b):
        assert np.abs(chroma - np.floor(chroma) - 0.5).min() >= 0.1
        c = np.rint(chroma).astype(np.int64)
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        for parity in (0, 1):
            classes = np.bincount(s[:, parity::2].ravel() % 4, minlength=4)
            assert (classes[1:] >= 1).all(), (parity, classes)
    # and the other colour fixtures are not all grey: chroma coefficients are present
    assert all(G[f"rgb_{n}_cb"].any() and G[f"rgb_{n}_cr"].any() for n in RGB if n != "dc_ties")
    assert not G["rgb_dc_ties_cb"].any() and not G["rgb_dc_ties_cr"].any()

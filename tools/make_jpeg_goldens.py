"""Generates tests/golden/jpeg_golden.npz: what libjpeg (through Pillow) makes of small seeded images -- the pin of the JPEG-domain
front end (frontend.transform_dct_jpeg / jpeg_planes_u8 / jpeg_quantised_dct on the host, the round_coeffs path of k_dct_frontend on
the device).  Runs where Pillow is; the tests read the npz only.

A baseline JPEG written with quality=100 has quantisation tables of ones, so the coefficients in the file ARE the quantised
coefficients of libjpeg's colour conversion -> 4:2:0 down-sampler -> "islow" integer DCT -> quantiser, which is what the reference
reads back with jpeg2dct.loads.  tests/jpeg_coef_ref.py (an entropy decoder, nothing of the product) recovers them.

Per colour image NAME (uint8 RGB, sides multiples of 16, none above 64 x 64):
    rgb_NAME_img   the array the front end is given
    rgb_NAME_jpeg  the bytes Pillow writes for img[..., ::-1] (the reference hands its RGB array to an encoder that expects BGR)
                   with quality=100, subsampling=2 (4:2:0)
    rgb_NAME_y / _cb / _cr   int16 [blocks_y, blocks_x, 64], natural order
Per grayscale plane NAME (mode L, no colour conversion, no down-sampling):
    gray_NAME_plane, gray_NAME_jpeg, gray_NAME_coef
and rgb_names, gray_names, pillow_version, libjpeg_turbo_version.  Data only."""
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def colour_images():
    rng = np.random.default_rng(20261)
    out = {}
    out["noise_wide"] = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)                 # non-square, 6 x 8 luma blocks
    out["noise_sq"] = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    out["noise_mcu"] = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)                  # one MCU: a 1 x 1 chroma grid
    yy, xx = np.mgrid[0:32, 0:48]
    out["ramp"] = np.stack([(yy * 5 + xx * 2) % 256, (xx * 5 + 7) % 256, (255 - yy * 3 - xx * 2) % 256], -1).astype(np.uint8)   # non-square too
    sat = rng.integers(0, 2, (32, 32, 3)) * 255
    sat[:16, :16] = (rng.integers(0, 2, (2, 2, 3)) * 255).repeat(8, 0).repeat(8, 1)       # whole saturated luma blocks beside pixel noise
    out["saturated"] = sat.astype(np.uint8)
    # flat 128; grey bumps leave Cb = Cr = 128 and move one block's luma sum by the bump: +-4 puts the DC term on +-0.5
    ties = np.full((32, 32, 3), 128, np.uint8)
    for (y, x), d in {(1, 2): 4, (3, 13): -4, (12, 5): 12, (9, 9): -12, (20, 20): 1, (21, 21): 3, (17, 30): -3, (18, 27): -1, (28, 3): 20, (30, 12): -20}.items():
        ties[y, x] = 128 + d
    out["dc_ties"] = ties
    # small chroma steps on grey: every 2 x 2 chroma sum class mod 4 at even and at odd output columns, where the down-sampler's
    # bias is 1 and 2.  The encoder sees channel 2 as red and channel 0 as blue: offsets 2a and 2c give Cr = 128 + a - 0.163 c and
    # Cb = 128 + c - 0.337 a, and with a <= 3, c <= 2 every pixel stays 0.16 or more away from a rounding boundary
    bias = np.full((32, 32, 3), 128, np.int64)
    bias[..., 0] += 2 * rng.integers(0, 3, (32, 32))
    bias[..., 2] += 2 * rng.integers(0, 4, (32, 32))
    out["chroma_bias"] = bias.astype(np.uint8)
    return out


def gray_planes():
    rng = np.random.default_rng(20262)
    out = {}
    out["noise"] = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    out["extremes"] = (rng.integers(0, 2, (40, 56)) * 255).astype(np.uint8)
    sat = np.full((40, 56), 128, np.uint8)
    sat[0:8, 0:8] = 0                                                                     # DC = -1024
    sat[0:8, 8:16] = 255                                                                  # DC = +1016
    sat[8:16, 0:8] = (np.indices((8, 8)).sum(0) % 2) * 255                                # checkerboard: the largest AC terms
    sat[8:16, 8:16] = np.where(np.arange(8) < 4, 0, 255)[None, :]                         # a vertical edge
    sat[16:24, 0:8] = np.where(np.arange(8) < 4, 255, 0)[:, None]                         # a horizontal edge
    sat[16:24, 8:24] = np.tile(np.array([0, 255], np.uint8), (8, 8))                      # columns alternating
    sat[24:32, 0:16] = np.tile(np.array([[255], [0]], np.uint8), (4, 16))                 # rows alternating
    sat[32:40, 32:40] = 0
    sat[32:40, 40:48] = 255
    out["saturated"] = sat
    ties = np.full((40, 56), 128, np.uint8)
    ties[0, :4] = 129                                                                     # block sum +4 -> DC +0.5
    ties[8, :4] = 127                                                                     # -4
    ties[3, 11] = 132
    ties[20, 20] = 124
    ties[16:24, 32:40] = 128 + np.where(np.arange(8) < 4, 1, -1)[None, :]                 # AC ties
    ties[33, 1:4] = 132                                                                   # +12 -> 1.5
    ties[35, 41:46] = 124                                                                 # -20 -> -2.5
    ties[24:32, 48:56] = rng.integers(126, 131, (8, 8))
    out["ties"] = ties
    return out


def encode_rgb(img):
    """the reference's call: the RGB array goes to an encoder that reads it as BGR, quality 100, 4:2:0"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, "JPEG", quality=100, subsampling=2)
    return buf.getvalue()


def encode_gray(plane):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(plane)).save(buf, "JPEG", quality=100)
    return buf.getvalue()


def versions():
    import PIL
    from PIL import features
    turbo = features.version_feature("libjpeg_turbo") if features.check_feature("libjpeg_turbo") else None
    return PIL.__version__, ("libjpeg-turbo %s" % turbo) if turbo else ("libjpeg %s" % features.version("jpg"))


def main():
    import jpeg_coef_ref as J
    z = {}
    rgb, gray = colour_images(), gray_planes()
    for name, img in rgb.items():
        assert img.shape[0] % 16 == 0 and img.shape[1] % 16 == 0 and max(img.shape[:2]) <= 64
        data = encode_rgb(img)
        comps = J.decode_coefficients(data)
        assert [(c.h, c.v) for c in comps] == [(2, 2), (1, 1), (1, 1)] and all((c.qtable == 1).all() for c in comps)
        z[f"rgb_{name}_img"] = img
        z[f"rgb_{name}_jpeg"] = np.frombuffer(data, np.uint8)
        for tag, c in zip(("y", "cb", "cr"), comps):
            z[f"rgb_{name}_{tag}"] = c.coef
    for name, plane in gray.items():
        data = encode_gray(plane)
        (c,) = J.decode_coefficients(data)
        assert (c.qtable == 1).all() and c.coef.shape == (plane.shape[0] // 8, plane.shape[1] // 8, 64)
        z[f"gray_{name}_plane"] = plane
        z[f"gray_{name}_jpeg"] = np.frombuffer(data, np.uint8)
        z[f"gray_{name}_coef"] = c.coef
    z["rgb_names"] = np.array(list(rgb))
    z["gray_names"] = np.array(list(gray))
    pv, jv = versions()
    z["pillow_version"] = np.array(pv)
    z["libjpeg_turbo_version"] = np.array(jv)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes; Pillow", pv, "libjpeg", jv)


if __name__ == "__main__":
    main()

"""Pillow's 8-bit two-pass resampler restated in numpy over ops.pillow_bicubic_tables, and the cases the CPU and GPU
tests of t2v_resample_crop_normalize_u8 share.

The restatement is the statement the kernel is written to (include/t2v.h): a horizontal pass rounded and saturated to
uint8 as clip8((2^21 + sum p*k) >> 22), then a vertical pass on those bytes with the same rule.  The CPU test holds it
to `Image.resize(..., Image.BICUBIC)` byte for byte; the GPU test holds the kernel to Pillow itself."""
import numpy as np

# (w, h) -> (w', h')
GEOMETRIES = [((37, 29), (52, 40)),
              ((61, 47), (24, 20)),       # 13 / 11 taps
              ((97, 33), (31, 33)),       # identity axis (rows)
              ((40, 40), (40, 52)),       # identity axis (columns)
              ((130, 90), (33, 23)),      # 17 taps
              ((19, 23), (76, 92)),
              ((384, 512), (396, 528))]


def geometry_id(g):
    return "%dx%d-%dx%d" % (g[0] + g[1])


def images(size, new_size, seed=0):
    """{name: uint8 [h, w, 3]}: uniform noise, and a 0/255 checkerboard whose overshoot saturates at both ends (cells of
    one pixel, or of four output pixels where the image shrinks: smaller cells would average out to grey)"""
    w, h = size
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cell = max(1, int(np.ceil(4 * max(w / new_size[0], h / new_size[1], 0.25))))
    checker = (((xx // cell + yy // cell) % 2) * 255).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "checker": np.stack([checker, 255 - checker, checker], -1)}


def _pass(img, tables, axis):
    """one pass along `axis` of uint8 [..., h, w, 3] in int64 (no product or sum here leaves int32's range)"""
    first, count, coef = tables
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(first),) + src.shape[1:], np.uint8)
    for i in range(len(first)):
        f, n = int(first[i]), int(count[i])
        acc = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), src[f:f + n], axes=(0, 0))
        out[i] = np.clip(acc >> 22, 0, 255)          # (numpy's >> on signed integers is arithmetic)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, new_size, tables_fn):
    """img uint8 [h, w, 3] -> [h', w', 3]: horizontal pass, then vertical pass on its bytes"""
    h, w, _ = img.shape
    nw, nh = new_size
    return _pass(_pass(img, tables_fn(w, nw), 1), tables_fn(h, nh), 0)

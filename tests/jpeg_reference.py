"""numpy restatement of the JPEG file the GPU writer produces (include/t2v_jpeg.h): baseline
sequential JFIF, 4:2:0, Annex K tables -- the bytes Pillow's `Image.save(format="JPEG", quality=Q)` writes.

    encode(image_u8[H,W,3|4], quality) -> Encoded(scan, file, stats)

Only the tables (text2video_amd.jpeg's Annex K constants, checked against Pillow's own DQT / DHT segments by
tests/test_cpu_jpeg.py) are shared with the code under test; the colour conversion, the down-sampling, the transform, the
quantisation and the entropy coder are written out again here, block by block, for the eye.  `stats` counts what the
symbol stream held (ZRL, EOB, blocks without EOB, categories, stuffed bytes, dummy blocks): the tests assert from it that
their cases reach every rule.
"""
import collections

import numpy as np

from text2video_amd import jpeg as J

Encoded = collections.namedtuple("Encoded", "scan file stats")


def _huffman(bits, vals):
    """(BITS, HUFFVAL) -> {symbol: (code, length)} (T.81 Annex C)"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


DC_TABLES = (_huffman(*J.DC_LUMA), _huffman(*J.DC_CHROMA))
AC_TABLES = (_huffman(*J.AC_LUMA), _huffman(*J.AC_CHROMA))


def ycc_planes(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample(c, mh, mw):
    """full-resolution chroma [H,W] -> [8 mh, 8 mw]: last column out to 16 mw, last row to an even height, 2x2 sums with
    the alternating bias, then the last DOWN-SAMPLED row out to 8 mh"""
    H, W = c.shape
    c = np.pad(c, ((0, H & 1), (0, 16 * mw - W)), mode="edge")
    bias = 1 + (np.arange(8 * mw) & 1)
    d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    return np.pad(d, ((0, 8 * mh - d.shape[0]), (0, 0)), mode="edge")


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """libjpeg's jfdctint.c ("islow") along the last axis; first: the row pass (results scaled up by 4), else the column
    pass (that factor and the 8x of the 1-D transform pair remain: the output is 8x the true DCT)"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def fdct(block):
    """[8,8] samples (already minus 128) -> [8,8] coefficients, 8x the true DCT"""
    rows = _fdct_pass(block.astype(np.int64), True)
    return _fdct_pass(rows.T, False).T


def quantise(coef, q):
    """[8,8] x natural-order table [64] -> [64] in zigzag order"""
    d = coef.reshape(64)
    v = np.sign(d) * ((np.abs(d) + 4 * q) // (8 * q))
    return v[J.ZIGZAG]


def _category(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def put_value(self, v, size):
        if size:
            self.put(v if v >= 0 else v + (1 << size) - 1, size)

    def bytes(self):
        pad = -self.n % 8
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        return acc.to_bytes(n // 8, "big")


def encode(image, quality=75):
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] in (3, 4)
    H, W = image.shape[:2]
    mh, mw = (H + 15) // 16, (W + 15) // 16
    bh, bw = (H + 7) // 8, (W + 7) // 8            # real Y blocks
    y, cb, cr = ycc_planes(image)
    yp = np.pad(y, ((0, 16 * mh - H), (0, 16 * mw - W)), mode="edge") - 128
    cbp, crp = downsample(cb, mh, mw) - 128, downsample(cr, mh, mw) - 128
    q_luma, q_chroma = (t.astype(np.int64) for t in J.quant_tables(quality))
    stats = collections.Counter()
    bits = _Bits()
    pred = [0, 0, 0]

    def code_block(zz, comp):
        tbl = 0 if comp == 0 else 1
        diff = int(zz[0]) - pred[comp]
        pred[comp] = int(zz[0])
        cat = _category(diff)
        stats["dc_category_max"] = max(stats["dc_category_max"], cat)
        bits.put(*DC_TABLES[tbl][cat])
        bits.put_value(diff, cat)
        run = 0
        for k in range(1, 64):
            v = int(zz[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*AC_TABLES[tbl][0xF0])
                stats["zrl"] += 1
                run -= 16
            size = _category(v)
            stats["ac_category_max"] = max(stats["ac_category_max"], size)
            bits.put(*AC_TABLES[tbl][(run << 4) | size])
            bits.put_value(v, size)
            run = 0
        if run:
            bits.put(*AC_TABLES[tbl][0x00])
            stats["eob"] += 1
        else:
            stats["no_eob"] += 1

    for my in range(mh):
        for mx in range(mw):
            last = None
            for k in range(4):
                by, bx = 2 * my + (k >> 1), 2 * mx + (k & 1)
                if by < bh and bx < bw:
                    last = quantise(fdct(yp[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]), q_luma)
                else:      # dummy: no AC, the DC of the block coded just before it
                    stats["dummy_corner" if (by >= bh and bx >= bw) else "dummy_bottom" if by >= bh else "dummy_right"] += 1
                    dc = last[0]
                    last = np.zeros(64, np.int64)
                    last[0] = dc
                code_block(last, 0)
            for comp, plane in ((1, cbp), (2, crp)):
                code_block(quantise(fdct(plane[8 * my:8 * my + 8, 8 * mx:8 * mx + 8]), q_chroma), comp)
    raw = bits.bytes()
    stats["stuffed"] = raw.count(b"\xff")
    stats["blocks"] = 6 * mh * mw
    scan = raw.replace(b"\xff", b"\xff\x00")
    return Encoded(scan, J.file_bytes(J.header(H, W, quality), scan), stats)


# ----------------------------------------------------------------------------------------------------------------------
# the cases both test files run: (kind, H, W, quality)
# ----------------------------------------------------------------------------------------------------------------------
CASES = [("noise", 8, 8, 75), ("noise", 21, 37, 75), ("noise", 40, 24, 75), ("noise", 40, 56, 75), ("noise", 48, 32, 75),
         ("constant", 16, 16, 75), ("smooth", 17, 49, 75), ("smooth", 24, 40, 75), ("smooth", 64, 88, 75),
         ("edges", 32, 40, 75), ("edges", 33, 31, 75), ("checker", 48, 32, 75),
         ("smooth", 64, 88, 90), ("noise", 32, 48, 30), ("checker", 48, 32, 100), ("noise", 40, 56, 100),
         ("edges", 33, 31, 90)]


def case_id(case):
    return "%s-%dx%d-q%d" % case


def make_image(kind, H, W, channels=3):
    """the uint8 [H,W,channels] image of a case (channel 3, where asked for, holds a value the encoder must ignore)"""
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        img = rng.integers(0, 256, (H, W, 3))
    elif kind == "constant":
        img = np.broadcast_to(np.array([200, 30, 90]), (H, W, 3))
    elif kind == "smooth":      # a gradient per channel with a little noise on it
        img = np.stack([xx * 255.0 / max(W - 1, 1), yy * 255.0 / max(H - 1, 1), (xx + yy) * 255.0 / max(H + W - 2, 1)], -1)
        img = img + rng.normal(0.0, 3.0, (H, W, 3))
    elif kind == "edges":       # saturated rectangles on black: hard edges off the block grid
        img = np.zeros((H, W, 3))
        img[H // 5:H // 2 + 3, W // 7:W // 2 + 1] = (255, 255, 255)
        img[H // 2 + 3:, W // 3:] = (255, 0, 0)
        img[:H // 4, W // 2 + 5:] = (0, 255, 255)
    elif kind == "checker":     # one-pixel black / white checkerboard
        img = np.broadcast_to((((yy + xx) & 1) * 255)[..., None], (H, W, 3))
    else:
        raise ValueError(kind)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if channels == 4:
        img = np.concatenate([img, np.full((H, W, 1), 0xA5, np.uint8)], -1)
    return np.ascontiguousarray(img)

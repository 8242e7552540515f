"""Plain integer restatement of the JPEG decoder of libt2v_jpegdec.so (include/t2v_jpeg_decode.h):

* `decode(blob)`: sequential Huffman decoding and libjpeg's reconstruction rules (integer dequantisation, the "islow" inverse
  DCT, fancy chroma up-sampling, the 16-bit fixed-point colour tables) -> the uint8 [H,W,3] array Pillow's
  `Image.open(...).convert("RGB")` gives.  tests/test_cpu_jpeg_decode.py pins it to the installed Pillow.
* `sync_rounds(blob)`: the self-synchronising scheme of the kernels, restated: per subsequence, the correction round after
  which its stored end state no longer changes.
* `CASES`, `make_image`, `pillow_file`: what both test files decode.

numpy only; nothing of the library."""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_reference as E  # noqa: E402

from text2video_amd import jpeg as J  # noqa: E402

SUBSEQ_BYTES = 128       # kSubseqBytes of jpeg_decode.hip: one thread's share of the scan (1024 bits)
ROUNDS = 22              # kRounds of jpeg_decode.hip: correction rounds per synchronisation launch


# ----------------------------------------------------------------------------------------------------------------------
# entropy decoding: one symbol walk, shared by the sequential decoder and the synchronisation scheme
# ----------------------------------------------------------------------------------------------------------------------
class Scan(object):
    """the entropy-coded bytes of one file with its decode tables.  A state is (B, o, b, k): the byte that holds the next
    bit (never the stuffed 00 behind an FF), the bit inside it (0 = most significant), the block index within the MCU and the
    zigzag index of the next coefficient."""

    def __init__(self, scan, tables, sampling):
        self.len = len(scan)
        self.a = bytes(scan) + b"\xff" * 32          # bytes past the length count as absent: they read as FF
        self.ny = (1, 2, 4)[sampling]
        self.bpm = self.ny + 2
        self.tables = []
        for t in range(4):
            raw = tables[J.TABLE_QUANT_BYTES + t * J.HUFF_BYTES:][:J.HUFF_BYTES]
            self.tables.append((np.frombuffer(raw, np.uint16, 256, J.HUFF_LOOK).tolist(),
                                np.frombuffer(raw, np.int32, 16, J.HUFF_MAXCODE).tolist(),
                                np.frombuffer(raw, np.int32, 16, J.HUFF_VALOFF).tolist(), raw[J.HUFF_VALS:]))

    def run(self, state, end, sink=None, first=0, nblocks=0):
        """decode the symbols that start before byte `end` -> (end state, blocks completed, invalid code seen while a block
        below `nblocks` was open).  sink(block ordinal, zigzag index, value) takes the coefficients (DC as a difference)."""
        B, o, b, k = state
        a, ny, bpm, tables = self.a, self.ny, self.bpm, self.tables
        n, bad = 0, False
        while B < end:
            w, q = 0, B
            for _ in range(5):                    # five data bytes from B on, stuffed 00s left out
                v = a[q]
                w = (w << 8) | v
                q += 2 if v == 0xFF else 1
            win = (w >> (8 - o)) & 0xFFFFFFFF     # the next 32 bits
            look, maxcode, valoff, vals = tables[(0 if b < ny else 2) + (1 if k else 0)]
            e = look[win >> 24]
            if e:
                length, sym = e >> 8, e & 255
            else:
                for length in range(9, 17):
                    code = win >> (32 - length)
                    if code <= maxcode[length - 1]:
                        sym = vals[code + valoff[length - 1]]
                        break
                else:
                    length, sym = 16, -1
            if sym < 0:                           # no such code: 16 bits are dropped, the block state stays
                used = 16
                bad = bad or first + n < nblocks
            else:
                s = sym & 15
                used = length + s
                value = 0
                if s:
                    value = (win << length & 0xFFFFFFFF) >> (32 - s)
                    if value < (1 << (s - 1)):
                        value -= (1 << s) - 1
                done = False
                if k == 0:                        # DC difference
                    if sink:
                        sink(first + n, 0, value)
                    k = 1
                else:
                    r = sym >> 4
                    if s:
                        k += r
                        if k > 63:
                            k = 63
                        if sink:
                            sink(first + n, k, value)
                        k += 1
                        done = k > 63
                    elif r == 15:                 # ZRL
                        k += 16
                        done = k > 63
                    else:                         # EOB (a run r < 15 without a value ends the block as well)
                        done = True
                if done:
                    k, b, n = 0, (b + 1) % bpm, n + 1
            o += used
            for j in range(o >> 3):
                B += 2 if (w >> (32 - 8 * j)) & 255 == 0xFF else 1
            o &= 7
        return (B, o, b, k), n, bad

    def blind(self, i):
        """the state subsequence i > 0 starts from when nothing is known: its first byte, or the one behind it where that
        is the 00 of an FF 00 pair"""
        B = i * SUBSEQ_BYTES
        return (B + (1 if self.a[B - 1] == 0xFF else 0), 0, 0, 0)


def sync_rounds(blob, subseq=SUBSEQ_BYTES):
    """-> [per subsequence: the correction round after which its end state is final].  Round 0 is the blind pass (subsequence
    0 starts from the true state); in round r subsequence i is decoded again from the end state round r - 1 left for i - 1.
    max() of the list is what kRounds must cover; the fixed point is the sequential decoder's chain by induction."""
    p = J.parse(blob)
    sc = Scan(blob[p.scan_offset:p.scan_offset + p.scan_length], p.tables, p.sampling)
    nsub = (sc.len + subseq - 1) // subseq
    memo = {}

    def f(i, state):
        if (i, state) not in memo:
            memo[i, state] = sc.run(state, min((i + 1) * subseq, sc.len))[:2]
        return memo[i, state]
    s = [f(0, (0, 0, 0, 0))] + [f(i, (i * subseq + (1 if sc.a[i * subseq - 1] == 0xFF else 0), 0, 0, 0)) for i in range(1, nsub)]
    last, r = [0] * nsub, 0
    while True:
        r += 1
        new = [s[0]] + [f(i, s[i - 1][0]) for i in range(1, nsub)]
        changed = [i for i in range(nsub) if new[i] != s[i]]
        if not changed:
            return last
        for i in changed:
            last[i] = r
        s = new


# ----------------------------------------------------------------------------------------------------------------------
# reconstruction (libjpeg: jidctint.c, jdsample.c, jdcolor.c)
# ----------------------------------------------------------------------------------------------------------------------
def _idct_pass(x, shift):
    """the eight outputs of one 1-D pass over the eight inputs x[0..7] (arrays), descaled by `shift`"""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return [(v + (1 << (shift - 1))) >> shift for v in out]


def idct(blocks):
    """int [N,8,8] dequantised coefficients -> uint8 [N,8,8] samples: columns first (CONST_BITS - PASS1_BITS), then rows
    (CONST_BITS + PASS1_BITS + 3), plus 128, clamped"""
    blocks = blocks.astype(np.int64)
    ws = np.stack(_idct_pass([blocks[:, r, :] for r in range(8)], 11), 1)
    out = np.stack(_idct_pass([ws[:, :, c] for c in range(8)], 18), 2)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def _upsample_h(c):
    """h2v1 fancy: [h, w] -> [h, 2w], neighbours clamped to the plane"""
    c = c.astype(np.int32)
    last = np.concatenate([c[:, :1], c[:, :-1]], 1)
    nxt = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int32)
    out[:, 0::2] = (3 * c + last + 1) >> 2
    out[:, 1::2] = (3 * c + nxt + 2) >> 2
    return out


def _upsample_hv(c):
    """h2v2 fancy: [h, w] -> [2h, 2w]"""
    c = c.astype(np.int32)
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int32)
    for parity, far in ((0, up), (1, down)):
        this = 3 * c + far
        last = np.concatenate([this[:, :1], this[:, :-1]], 1)
        nxt = np.concatenate([this[:, 1:], this[:, -1:]], 1)
        out[parity::2, 0::2] = (3 * this + last + 8) >> 4
        out[parity::2, 1::2] = (3 * this + nxt + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


class Decoded(object):
    __slots__ = ("rgb", "corrupt", "nblocks", "blocks_seen")


def decode(blob):
    """the file -> Decoded: .rgb uint8 [H,W,3]; .corrupt: an invalid code, a stream that ends early or a wrong block count"""
    p = J.parse(blob)
    H, W, sampling = p.H, p.W, p.sampling
    hs, vs = ((1, 1), (2, 1), (2, 2))[sampling]
    mw, mh = (W + 8 * hs - 1) // (8 * hs), (H + 8 * vs - 1) // (8 * vs)
    sc = Scan(blob[p.scan_offset:p.scan_offset + p.scan_length], p.tables, sampling)
    nblocks = mw * mh * sc.bpm
    coef = np.zeros((nblocks, 64), np.int32)

    def sink(ordinal, k, value):
        if ordinal < nblocks:
            coef[ordinal, J.ZIGZAG[k]] = value
    state, n, bad = sc.run((0, 0, 0, 0), sc.len, sink, 0, nblocks)
    out = Decoded()
    out.nblocks, out.blocks_seen = nblocks, n
    out.corrupt = bool(bad or n != nblocks or state[2:] != (0, 0))
    quant = np.frombuffer(p.tables, np.uint16, 192).reshape(3, 64).astype(np.int32)
    coef = coef.reshape(mh * mw, sc.bpm, 64)
    planes = []
    for c in range(3):
        mine = coef[:, :sc.ny] if c == 0 else coef[:, sc.ny + c - 1:sc.ny + c]
        flat = mine.reshape(-1, 64).copy()
        flat[:, 0] = np.cumsum(flat[:, 0])
        px = idct((flat * quant[c]).reshape(-1, 8, 8))
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        # [mcu row, mcu column, block row, block column, 8, 8] -> the plane
        px = px.reshape(mh, mw, cv, ch, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * cv * 8, mw * ch * 8)
        planes.append(px)
    cw, chh = (W + hs - 1) // hs, (H + vs - 1) // vs      # the chroma planes' real extent
    y = planes[0][:H, :W]
    up = {0: lambda c: c, 1: _upsample_h, 2: _upsample_hv}[sampling]
    cb, cr = (up(pl[:chh, :cw])[:H, :W] for pl in planes[1:])
    out.rgb = ycc_to_rgb(y, cb, cr)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the cases both test files decode: (kind, H, W, quality, subsampling, optimize)
# ----------------------------------------------------------------------------------------------------------------------
CASES = [("noise", 8, 8, 75, 0, False), ("noise", 8, 8, 75, 1, False), ("noise", 8, 8, 75, 2, False),
         ("smooth", 16, 16, 75, 2, False), ("smooth", 17, 13, 75, 2, False), ("edges", 33, 31, 90, 2, False),
         ("smooth", 24, 40, 75, 2, False), ("noise", 48, 40, 75, 1, False), ("noise", 40, 56, 75, 0, False),
         ("edges", 33, 31, 75, 1, False), ("smooth", 17, 13, 75, 0, True),
         ("smooth", 64, 88, 90, 2, True), ("constant", 64, 64, 75, 2, False), ("noise", 16, 16, 100, 2, False),
         ("smooth", 160, 96, 95, 2, False), ("pose", 160, 96, 75, 2, False),
         ("smooth", 2048, 8, 75, 2, False), ("smooth", 8, 2048, 75, 2, False),
         # 262 subsequences: a second workgroup, whose first threads are corrected from the first one's settled states
         ("noise", 200, 120, 80, 0, False)]
# three files of one geometry with their own tables and lengths
BATCH = [("smooth", 40, 56, 75, 2, False), ("smooth", 40, 56, 90, 2, True), ("noise", 40, 56, 30, 2, False)]
# does not synchronise within ROUNDS: blocks without EOB, 16-bit codes (status bit 0, the Pillow fallback)
FALLBACK = ("noise", 64, 64, 100, 2, False)
BATCH_FALLBACK = [("smooth", 64, 64, 75, 2, False), FALLBACK, ("edges", 64, 64, 90, 2, True)]
# what kRounds rests on: frame-like pictures at 512 x 512
FRAME_CASES = [("smooth", 512, 512, 75, 2, False), ("smooth", 512, 512, 95, 2, False), ("pose", 512, 512, 75, 2, False),
               ("pose", 512, 512, 95, 2, False)]


def case_id(case):
    return "%s-%dx%d-q%d-s%d%s" % (case[:5] + ("-opt" if case[5] else "",))


def make_image(kind, H, W):
    if kind != "pose":
        return E.make_image(kind, H, W)
    # black with thin coloured lines and small discs: a rendered skeleton
    rng = np.random.default_rng(H * 1000 + W + 7)
    img = np.zeros((H, W, 3), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    pts = np.stack([rng.uniform(0.1, 0.9, 14) * H, rng.uniform(0.1, 0.9, 14) * W], 1)
    for i in range(13):
        (y0, x0), (y1, x1) = pts[i], pts[i + 1]
        colour = rng.integers(64, 256, 3)
        d = np.hypot(y1 - y0, x1 - x0)
        t = np.clip(((yy - y0) * (y1 - y0) + (xx - x0) * (x1 - x0)) / (d * d), 0, 1)
        dist = np.hypot(yy - (y0 + t * (y1 - y0)), xx - (x0 + t * (x1 - x0)))
        img[dist <= max(1.0, min(H, W) / 200.0)] = colour
        img[np.hypot(yy - y0, xx - x0) <= max(1.5, min(H, W) / 120.0)] = colour[::-1]
    return img


_files = {}


def pillow_file(case):
    """the bytes Pillow writes for a case: computed once, shared"""
    from PIL import Image
    if case not in _files:
        kind, H, W, q, sub, opt = case
        buf = io.BytesIO()
        Image.fromarray(make_image(kind, H, W)).save(buf, format="JPEG", quality=q, subsampling=sub, optimize=opt)
        _files[case] = buf.getvalue()
    return _files[case]


def pillow_rgb(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.asarray(im.convert("RGB"))

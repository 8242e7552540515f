"""The PNG writer's format, restated in numpy with integers only (include/t2v_png.h).  This file is
the definition: libt2v_png.so has to write these bytes.

    file     = signature, IHDR (8-bit truecolour, no interlace), ONE IDAT, IEND; no ancillary chunk
    IDAT     = 78 01, the Deflate stream, Adler-32 of the filtered bytes
    filtered = per row 1 filter byte + 3W bytes.  All five filter types are formed (the row above row 0 is zeros); the
               type whose residuals, read as signed bytes (min(v, 256 - v)), have the smallest sum wins, the lowest type
               on a tie.
    blocks   = one dynamic-Huffman block (BTYPE 2) per band of 8 rows (the last band may be shorter), bit-contiguous,
               BFINAL on the last.
    tokens   = per band, every maximal run of equal bytes (runs end at the band's end): its first byte a literal, then,
               with R bytes left, chunks of min(258, rest) bytes while the rest is >= 3, each a match (length, distance 1);
               a rest of 1 or 2 bytes is literals.  No other matches.
    codes    = literal/length: code_lengths(histogram with the end-of-block symbol, 15); distance: the one code 0 with
               length 1 if the band has a match, else one code of length 0 (RFC 1951, 3.2.7); the HLIT + 1 lengths are
               run-length coded by rle_code_lengths() and that alphabet gets code_lengths(., 7).
    code_lengths(counts, limit): the used symbols sorted by (count, symbol) ascending; the in-place minimum-redundancy
               algorithm of Moffat and Katajainen on the sorted counts gives the number of codes of every length; lengths
               above `limit` are folded into `limit` and the Kraft sum is repaired by, while it exceeds 1, taking one code
               off `limit` and moving one code of the longest length below `limit` that has one down a level together
               with it (two codes one level deeper); the lengths are then dealt out shortest first to the symbols from
               the END of the sorted order (most frequent first).  One used symbol gets length 1.
    canonical codes as RFC 1951 3.2.2, written bit-reversed into an LSB-first stream.
"""
import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BAND_ROWS = 8
MAX_DIM = 2048
NSYM = 286
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# length 3..258 -> (symbol, extra bits, extra value)
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
LEN_SYM = np.zeros(259, np.int64)
LEN_XBITS = np.zeros(259, np.int64)
LEN_XVAL = np.zeros(259, np.int64)
for _n in range(3, 259):
    _i = max(i for i in range(29) if _LEN_BASE[i] <= _n)
    LEN_SYM[_n], LEN_XBITS[_n], LEN_XVAL[_n] = 257 + _i, _LEN_EXTRA[_i], _n - _LEN_BASE[_i]

_CRC_TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32(data):
    c = 0xFFFFFFFF
    t = _CRC_TABLE
    for b in data:
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(data):
    a, b = 1, 0
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    for lo in range(0, len(d), 4096):
        c = d[lo:lo + 4096]
        n = len(c)
        b = (b + n * a + int((c * np.arange(n, 0, -1)).sum())) % 65521
        a = (a + int(c.sum())) % 65521
    return (b << 16) | a


def chunk(kind, payload):
    return len(payload).to_bytes(4, "big") + kind + payload + crc32(kind + payload).to_bytes(4, "big")


# ----------------------------------------------------------------------------------------------------------------------
# filtering
# ----------------------------------------------------------------------------------------------------------------------
def filter_rows(img):
    """[H,W,>=3] uint8 -> (filtered uint8 [H, 1+3W], the filter types [H])"""
    H, W = img.shape[:2]
    x = img[:, :, :3].reshape(H, 3 * W).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, 3:] = b[:, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255           # [5,H,3W]
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                                 # [5,H]
    types = np.argmin(cost, axis=0)                                                 # the lowest type on a tie
    out = np.empty((H, 1 + 3 * W), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out, types


# ----------------------------------------------------------------------------------------------------------------------
# codes
# ----------------------------------------------------------------------------------------------------------------------
def _minimum_redundancy(A):
    """Moffat & Katajainen, in place: A = the counts, ascending, n >= 2 -> A = the code lengths (non-increasing)"""
    n = len(A)
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or A[root] < A[leaf]:
            A[nxt] = A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] = A[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] += A[leaf]
            leaf += 1
    A[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            used += 1
            root -= 1
        while avbl > used:
            A[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    return A


def code_lengths(counts, limit):
    """-> (lengths per symbol, the longest length before limiting)"""
    counts = [int(c) for c in counts]
    order = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    lengths = [0] * len(counts)
    if not order:
        return lengths, 0
    if len(order) == 1:
        lengths[order[0][1]] = 1
        return lengths, 1
    depth = _minimum_redundancy([c for c, _ in order])
    unlimited = max(depth)
    num = [0] * (max(unlimited, limit) + 1)
    for d in depth:
        num[d] += 1
    for i in range(limit + 1, len(num)):
        num[limit] += num[i]
    total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
    while total != 1 << limit:
        num[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    j = len(order)
    for i in range(1, limit + 1):
        for _ in range(num[i]):
            j -= 1
            lengths[order[j][1]] = i
    assert j == 0
    return lengths, unlimited


def canonical_codes(lengths):
    """RFC 1951 3.2.2, then every code bit-reversed (the stream is LSB-first, Huffman codes go MSB-first)"""
    top = max(lengths) if len(lengths) else 0
    bl = [0] * (top + 2)
    for n in lengths:
        bl[n] += 1
    bl[0] = 0
    nxt, code = [0] * (top + 2), 0
    for bits in range(1, top + 1):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            c = nxt[n]
            nxt[n] += 1
            out[s] = int(format(c, "0%db" % n)[::-1], 2)
    return out


def rle_code_lengths(seq):
    """the fixed greedy rule -> [(symbol, extra bits, extra value)].  A run of zeros: 18 for min(run, 138) while the run is
    >= 11, then 17 if >= 3 are left, else single zeros.  A run of a length v > 0: v once, then 16 for min(rest, 6) while
    the rest is >= 3, then the rest as single v."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        r, i = j - i, j
        if v == 0:
            while r >= 11:
                m = min(r, 138)
                out.append((18, 7, m - 11))
                r -= m
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                m = min(r, 6)
                out.append((16, 2, m - 3))
                r -= m
        out += [(v, 0, 0)] * r
    return out


class Bits:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, v, n):
        self.vals.append(v)
        self.lens.append(n)


def block_header(final, ll_len, has_match):
    """-> Bits of BFINAL .. the coded code lengths"""
    hlit = 257
    for s in range(257, NSYM):
        if ll_len[s]:
            hlit = s + 1
    seq = list(ll_len[:hlit]) + [1 if has_match else 0]
    rle = rle_code_lengths(seq)
    cl_count = [0] * 19
    for s, _, _ in rle:
        cl_count[s] += 1
    cl_len, _ = code_lengths(cl_count, 7)
    cl_code = canonical_codes(cl_len)
    hclen = 4
    for i, s in enumerate(CL_ORDER):
        if cl_len[s]:
            hclen = max(hclen, i + 1)
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(0, 5)
    b.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        b.put(cl_len[s], 3)
    for s, xb, xv in rle:
        b.put(cl_code[s], cl_len[s])
        if xb:
            b.put(xv, xb)
    return b


def tokens_of(flat, band_of):
    """flat: the filtered bytes; band_of: the band of every byte -> per emitted token its position, its symbol and its
    match length (0: a literal)"""
    n = len(flat)
    start = np.ones(n, bool)
    start[1:] = (flat[1:] != flat[:-1]) | (band_of[1:] != band_of[:-1])
    first = np.flatnonzero(start)
    run_len = np.diff(np.append(first, n))
    run = np.cumsum(start) - 1
    j = np.arange(n) - first[run]
    R = run_len[run] - 1
    k = j - 1
    c = k - k % 258
    len_c = np.minimum(258, R - c)
    lit = (j == 0) | (len_c < 3)
    match = (j > 0) & (len_c >= 3) & (k == c)
    pos = np.flatnonzero(lit | match)
    length = np.where(match[pos], len_c[pos], 0)
    sym = np.where(length > 0, LEN_SYM[length], flat[pos].astype(np.int64))
    return pos, sym, length


def pack_bits(vals, lens):
    """LSB-first: value i occupies lens[i] bits from bit sum(lens[:i]) -> (bytes, the number of bits)"""
    vals, lens = np.asarray(vals, np.int64), np.asarray(lens, np.int64)
    total = int(lens.sum())
    off = np.cumsum(lens) - lens
    idx = np.repeat(np.arange(len(vals)), lens)
    bit = np.arange(total) - off[idx]
    return np.packbits(((vals[idx] >> bit) & 1).astype(np.uint8), bitorder="little").tobytes(), total


class Encoded:
    """file; filtered: the bytes Deflate codes; deflate: the raw stream; payload: the IDAT's; filters [H]; stats"""


def encode(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4)
    H, W = img.shape[:2]
    assert 1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM
    filt, types = filter_rows(img)
    flat = filt.reshape(-1)
    row = 1 + 3 * W
    band_of = np.arange(len(flat)) // (row * BAND_ROWS)
    nbands = (H + BAND_ROWS - 1) // BAND_ROWS
    pos, sym, length = tokens_of(flat, band_of)
    tband = band_of[pos]
    hist = np.bincount(tband * NSYM + sym, minlength=nbands * NSYM).reshape(nbands, NSYM)
    hist[:, 256] = 1
    vals, lens = [], []
    stats = {"unlimited_max": 0, "matches": int((length > 0).sum()), "literals": int((length == 0).sum()),
             "two_symbol_bands": 0, "no_match_bands": 0, "header_bits_max": 0, "max_match": int(length.max(initial=0))}
    for b in range(nbands):
        sel = tband == b
        ll_len, unlimited = code_lengths(hist[b], 15)
        stats["unlimited_max"] = max(stats["unlimited_max"], unlimited)
        has_match = bool((length[sel] > 0).any())
        stats["no_match_bands"] += not has_match
        ll_code = np.array(canonical_codes(ll_len), np.int64)
        ll_len = np.array(ll_len, np.int64)
        head = block_header(b == nbands - 1, list(ll_len), has_match)
        stats["header_bits_max"] = max(stats["header_bits_max"], sum(head.lens))
        vals += head.vals
        lens += head.lens
        s, n = sym[sel], length[sel]
        m = n > 0
        # a match: the length code, its extra bits, the one-bit distance code 0
        vals += (ll_code[s] | np.where(m, LEN_XVAL[n] << ll_len[s], 0)).tolist()
        lens += (ll_len[s] + np.where(m, LEN_XBITS[n] + 1, 0)).tolist()
        vals.append(int(ll_code[256]))
        lens.append(int(ll_len[256]))
    deflate, nbits = pack_bits(vals, lens)
    e = Encoded()
    e.filtered, e.filters, e.deflate, e.stats = flat.tobytes(), types, deflate, stats
    e.payload = b"\x78\x01" + deflate + adler32(e.filtered).to_bytes(4, "big")
    ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
    e.file = SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", e.payload) + chunk(b"IEND", b"")
    return e


def file_capacity(H, W):
    """include/t2v_png.h, t2v_png_file_capacity"""
    nbands = (H + BAND_ROWS - 1) // BAND_ROWS
    bits = nbands * (74 + 287 * 7 + 15) + 15 * H * (1 + 3 * W)
    return 63 + (bits + 7) // 8


def chunks_of(blob):
    """[(type, payload, crc)] of a PNG file"""
    assert blob[:8] == SIGNATURE
    out, i = [], 8
    while i < len(blob):
        n = int.from_bytes(blob[i:i + 4], "big")
        out.append((blob[i + 4:i + 8], blob[i + 8:i + 8 + n], int.from_bytes(blob[i + 8 + n:i + 12 + n], "big")))
        i += 12 + n
    assert i == len(blob)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the cases both test files share
# ----------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("mixed", 1, 1), ("mixed", 1, 7), ("mixed", 7, 1), ("mixed", 8, 5), ("mixed", 9, 5), ("mixed", 17, 3),
         ("zero", 24, 90), ("colour", 16, 100), ("noise", 33, 65), ("fibonacci", 8, 175), ("crop", 128, 128), ("pose", 64, 64)]
BIG_CASE = ("tiled", 512, 512)


def case_id(case):
    return "%s-%dx%d" % case


def _fibonacci_rows(H, W):
    """Bytes whose counts are Fibonacci numbers, no two neighbours equal: with filter 0 on every row the band's histogram
    needs a 16-bit code before limiting.  Small magnitudes (0, 1, 255, 2, 254, ...) keep filter 0 the cheapest."""
    n = 3 * W * H
    fib = [1, 2]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    fib = fib[::-1]                                   # 1597, 987, ..., 2, 1
    fib[0] += n - sum(fib)
    assert fib[0] * 2 <= n + 1
    values = [0] + [v for i in range(1, 9) for v in (i, 256 - i)]
    seq = np.concatenate([np.full(c, values[i], np.uint8) for i, c in enumerate(fib)])
    out = np.empty(n, np.uint8)
    half = (n + 1) // 2
    out[0::2] = seq[:half]
    out[1::2] = seq[half:]
    return out.reshape(H, W, 3)


_crop = {}


def make_image(kind, H, W, cs=3):
    """the image of a case; cs 4 adds a fourth channel of random bytes, which the writer ignores"""
    rng = np.random.default_rng(H * 4099 + W)
    if kind == "zero":
        img = np.zeros((H, W, 3), np.uint8)
    elif kind == "colour":
        img = np.empty((H, W, 3), np.uint8)
        img[:] = (200, 17, 99)
    elif kind == "noise":
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "mixed":      # a ramp with a little noise: the rows choose different filters
        y, x = np.mgrid[0:H, 0:W]
        img = ((3 * x + 5 * y)[..., None] * np.array([1, 2, 3]) + rng.integers(0, 3, (H, W, 3))).astype(np.uint8)
    elif kind == "fibonacci":
        img = _fibonacci_rows(H, W)
    elif kind == "crop":
        if "crop" not in _crop:
            _crop["crop"] = np.load(os.path.join(GOLD, "png_crop_fadg0.npy"))
        img = _crop["crop"][:H, :W]
    elif kind == "pose":
        if "pose" not in _crop:
            _crop["pose"] = np.load(os.path.join(GOLD, "pose_maps_fadg0.npz"))["maps"][0]
        m = _crop["pose"]
        ys, xs = np.nonzero(m.any(axis=2))
        y0 = int(min(max(int(np.median(ys)) - H // 2, 0), m.shape[0] - H))
        x0 = int(min(max(int(np.median(xs)) - W // 2, 0), m.shape[1] - W))
        img = m[y0:y0 + H, x0:x0 + W]
    elif kind == "tiled":
        crop = make_image("crop", 128, 128)
        img = np.tile(crop, ((H + 127) // 128, (W + 127) // 128, 1))[:H, :W].copy()
        img[H // 2:] = (img[H // 2:].astype(np.int64) + rng.integers(-2, 3, img[H // 2:].shape)).clip(0, 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    img = np.ascontiguousarray(img)
    if cs == 4:
        img = np.concatenate([img, np.random.default_rng(7).integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
    return img

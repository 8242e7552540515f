"""Host side of the GPU JPEG writer (ops.jpeg_encode_u8, include/t2v_jpeg.h): everything of the file that does not depend
on the pixels.  No GPU, no torch, no library: numpy only.

The file is the one Pillow's `Image.save(path, "JPEG", quality=Q)` writes for an RGB image:
baseline sequential JFIF, 8 bit, Y 2x2 / Cb 1x1 / Cr 1x1, one interleaved scan, the ITU-T T.81 Annex K quantisation
tables scaled by the IJG quality rule and the Annex K Huffman tables.  `header()` is every byte before the entropy-coded
scan, `file_bytes()` appends the scan the kernels produced and the EOI marker.
"""
import struct

import numpy as np

# Annex K.1 / K.2 in natural (row-major) order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int32)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int32)

# ZIGZAG[k]: natural index of the k-th coefficient in coding order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
    62, 63], np.int32)

# Annex K.3: (BITS[16], HUFFVAL) of the four tables, in the order the DHT segments are written: DC 0, AC 0, DC 1, AC 1
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
    "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
HUFFMAN_TABLES = ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))

SOI, EOI = b"\xff\xd8", b"\xff\xd9"


def quant_tables(quality=75):
    """(luma, chroma): the two quantisation tables at `quality` (1..100), int32 [64] in natural order:
    q = clamp((base * s + 50) / 100, 1, 255) with s = 5000 / Q below 50 and 200 - 2 Q from 50 on (integer division)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("jpeg: quality %r is not in 1..100" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int32) for base in (BASE_LUMA, BASE_CHROMA))


def _segment(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


def header(H, W, quality=75):
    """Every byte of the file before the scan: SOI, APP0 (JFIF 1.01, no density unit, 1:1), one DQT per table, SOF0, one
    DHT per table, SOS.  623 bytes for every geometry and quality."""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("jpeg: %dx%d is not a JPEG frame size" % (H, W))
    out = [SOI, _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for i, t in enumerate(quant_tables(quality)):
        out.append(_segment(0xDB, bytes([i]) + bytes(int(v) for v in t[ZIGZAG])))
    # 8 bit, H, W, three components: (id, sampling h<<4 | v, quantisation table)
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, (bits, vals) in HUFFMAN_TABLES:
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + vals))
    # three components: (id, DC table << 4 | AC table); spectral selection 0..63, no successive approximation
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def file_bytes(header, scan):      # noqa: A002 -- the argument is what header() returned
    """The finished file: header + entropy-coded scan + EOI."""
    return b"".join((header, bytes(scan), EOI))


# ----------------------------------------------------------------------------------------------------------------------
# Reading: what the GPU decoder (ops.jpeg_decode_u8, include/t2v_jpeg_decode.h) needs of a file.  DESIGN.md section 4.11.
# ----------------------------------------------------------------------------------------------------------------------
TABLE_QUANT_BYTES = 3 * 64 * 2                   # uint16 [3][64], natural order: the table of component 0, 1, 2
HUFF_LOOK, HUFF_MAXCODE, HUFF_VALOFF, HUFF_VALS = 0, 512, 576, 640      # offsets inside one Huffman decode table
HUFF_BYTES = 896
TABLE_BYTES = TABLE_QUANT_BYTES + 4 * HUFF_BYTES       # t2v_jpegdec_table_bytes()
SAMPLINGS = {(1, 1): 0, (2, 1): 1, (2, 2): 2}          # Y's (h, v) -> Pillow's `subsampling` number


class JpegUnsupported(ValueError):
    """parse(): the file is not one the GPU decoder takes; .reason says why (Pillow decodes it)"""

    def __init__(self, reason):
        ValueError.__init__(self, "jpeg: " + reason)
        self.reason = reason


class Parsed(object):
    """H, W; sampling (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0); tables: the TABLE_BYTES blob; scan_offset, scan_length: the
    entropy-coded bytes between the SOS header and EOI inside the file"""
    __slots__ = ("H", "W", "sampling", "tables", "scan_offset", "scan_length")

    def __init__(self, H, W, sampling, tables, scan_offset, scan_length):
        self.H, self.W, self.sampling, self.tables = H, W, sampling, tables
        self.scan_offset, self.scan_length = scan_offset, scan_length


def huffman_decode_table(bits, vals):
    """One DHT table -> its HUFF_BYTES decode table: uint16 look[256] (length << 8 | symbol for the codes of at most 8
    bits, indexed by the next 8 bits; 0 = longer), int32 maxcode[16] (largest code of length l at [l - 1], -1 = none),
    int32 valoff[16] (index of a length-l code's symbol = code + valoff[l - 1]), uint8 vals[256]."""
    bits = [int(b) for b in bits]
    vals = bytes(vals)
    if len(bits) != 16 or sum(bits) != len(vals) or len(vals) > 256:
        raise JpegUnsupported("a Huffman table of %d codes for %d symbols" % (sum(bits), len(vals)))
    look = np.zeros(256, np.uint16)
    maxcode = np.full(16, -1, np.int32)
    valoff = np.zeros(16, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if code + n > (1 << length):
            raise JpegUnsupported("a Huffman table with more codes than %d bits hold" % length)
        if n:
            valoff[length - 1] = k - code
            maxcode[length - 1] = code + n - 1
            if length <= 8:
                for j in range(n):
                    first = (code + j) << (8 - length)
                    look[first:first + (1 << (8 - length))] = (length << 8) | vals[k + j]
        code, k = (code + n) << 1, k + n
    return look.tobytes() + maxcode.tobytes() + valoff.tobytes() + vals.ljust(256, b"\0")


def table_blob(quant, huff):
    """quant: three int [64] tables in natural order (of Y, Cb, Cr); huff: four (bits, vals) in the order DC of Y, AC of Y,
    DC of the chroma components, AC of the chroma components -> the TABLE_BYTES blob of one image"""
    q = np.stack([np.asarray(t).reshape(64) for t in quant]).astype(np.uint16)
    blob = q.tobytes() + b"".join(huffman_decode_table(b, v) for b, v in huff)
    assert len(blob) == TABLE_BYTES
    return blob


def parse(data):
    """The geometry, sampling, table blob and scan position of a JPEG file (bytes) -> Parsed.  Raises JpegUnsupported(reason)
    for anything but: baseline SOF0, 8 bit, three components Y / Cb / Cr sampled 4:4:4, 4:2:2 (Y 2x1) or 4:2:0 (Y 2x2), JFIF
    or no application marker (an Adobe APP14 is refused), 8-bit quantisation tables, one interleaved scan 0..63 and no
    restart interval."""
    data = bytes(data)
    if data[:2] != SOI:
        raise JpegUnsupported("no SOI marker: not a JPEG file")
    i, n = 2, len(data)
    quant, huff, frame = {}, {}, None
    while True:
        if i + 4 > n:
            raise JpegUnsupported("the file ends before a scan")
        if data[i] != 0xFF:
            raise JpegUnsupported("no marker at byte %d" % i)
        marker = data[i + 1]
        if marker == 0xFF:          # fill byte
            i += 1
            continue
        length = struct.unpack(">H", data[i + 2:i + 4])[0]
        seg = data[i + 4:i + 2 + length]
        if length < 2 or i + 2 + length > n:
            raise JpegUnsupported("a segment runs past the end of the file")
        i += 2 + length
        if marker == 0xC0:
            if frame is not None:
                raise JpegUnsupported("two frame headers")
            if len(seg) < 6 or seg[0] != 8:
                raise JpegUnsupported("%d-bit samples (8 only)" % (seg[0] if seg else 0))
            H, W, nc = struct.unpack(">HHB", seg[1:6])
            if nc != 3 or len(seg) != 6 + 3 * nc:
                raise JpegUnsupported("%d components (Y / Cb / Cr only: grey and CMYK files go to Pillow)" % nc)
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)]
            if bytes(c[0] for c in comps) == b"RGB":
                raise JpegUnsupported("components named R, G, B: not YCbCr")
            sampling = SAMPLINGS.get(comps[0][1:3])
            if sampling is None or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
                raise JpegUnsupported("sampling factors %s (4:4:4, 4:2:2 or 4:2:0 only)" % ", ".join("%dx%d" % c[1:3] for c in comps))
            if H < 1 or W < 1:
                raise JpegUnsupported("a frame of %dx%d" % (H, W))
            frame = (H, W, sampling, comps)
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            raise JpegUnsupported({0xC2: "a progressive file (SOF2)", 0xC1: "extended sequential (SOF1)"}.get(
                marker, "frame type SOF%d" % (marker - 0xC0)) + ": baseline SOF0 only")
        elif marker == 0xCC:
            raise JpegUnsupported("arithmetic coding")
        elif marker == 0xDB:
            j = 0
            while j < len(seg):
                if seg[j] >> 4:
                    raise JpegUnsupported("a 16-bit quantisation table")
                if j + 65 > len(seg):
                    raise JpegUnsupported("a short DQT segment")
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[j + 1:j + 65], np.uint8)
                quant[seg[j] & 15] = t
                j += 65
        elif marker == 0xC4:
            j = 0
            while j < len(seg):
                if j + 17 > len(seg):
                    raise JpegUnsupported("a short DHT segment")
                bits = tuple(seg[j + 1:j + 17])
                if j + 17 + sum(bits) > len(seg):
                    raise JpegUnsupported("a short DHT segment")
                huff[seg[j]] = (bits, seg[j + 17:j + 17 + sum(bits)])
                j += 17 + sum(bits)
        elif marker == 0xDD:
            if struct.unpack(">H", seg[:2])[0]:
                raise JpegUnsupported("a restart interval (DRI)")
        elif marker == 0xEE and seg[:5] == b"Adobe":
            raise JpegUnsupported("an Adobe APP14 marker (its colour transform flag decides the conversion)")
        elif marker == 0xDA:
            break
        elif marker == 0xD9 or 0xD0 <= marker <= 0xD7:
            raise JpegUnsupported("marker FF%02X before a scan" % marker)
        # APPn, COM and the rest: skipped
    if frame is None:
        raise JpegUnsupported("a scan before the frame header")
    H, W, sampling, comps = frame
    if len(seg) != 10 or seg[0] != 3:
        raise JpegUnsupported("a scan of %d components (one interleaved scan of three only)" % (seg[0] if seg else 0))
    if tuple(seg[7:10]) != (0, 63, 0):
        raise JpegUnsupported("a scan of coefficients %d..%d, approximation %02x" % tuple(seg[7:10]))
    if [seg[1 + 2 * c] for c in range(3)] != [c[0] for c in comps]:
        raise JpegUnsupported("scan components in another order than the frame's")
    sel = [seg[2 + 2 * c] for c in range(3)]
    if sel[1] != sel[2]:
        raise JpegUnsupported("Cb and Cr with different Huffman tables")
    try:
        q = [quant[c[3]] for c in comps]
        h = [huff[sel[0] >> 4], huff[0x10 | (sel[0] & 15)], huff[sel[1] >> 4], huff[0x10 | (sel[1] & 15)]]
    except KeyError as e:
        raise JpegUnsupported("table %s is not defined" % (e.args[0],))
    a = np.frombuffer(data, np.uint8, offset=i)
    marks = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0))
    if not len(marks):
        raise JpegUnsupported("no EOI marker behind the scan")
    m = int(marks[0])
    if a[m + 1] != 0xD9:
        raise JpegUnsupported("marker FF%02X inside or behind the scan (restart markers, a second scan)" % a[m + 1])
    return Parsed(H, W, sampling, table_blob(q, h), i, m)

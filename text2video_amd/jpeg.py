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

/*
 * t2v_jpeg_decode.h -- C ABI of libt2v_jpegdec.so: a baseline JPEG decoder for the MI355X (gfx950) that gives, byte for
 * byte, the RGB array libjpeg-turbo / Pillow's Image.open(...).convert("RGB") gives for the same file.
 *
 * The third stand-alone library beside libt2v_hip.so (t2v.h) and libt2v_jpeg.so (t2v_jpeg.h, the encoder): nothing of
 * either, no context object; raw device pointers and a hipStream_t in, pixels out.  The host reads the markers
 * (text2video_amd/jpeg.py: parse()) and hands over what the kernels need: the entropy-coded scan as it stands in the file
 * and one table blob per image.
 *
 * Format (DESIGN.md section 4.11 has the rules in full): baseline sequential SOF0, 8 bit, Y / Cb / Cr with Y sampled
 * 1x1, 2x1 or 2x2, one interleaved scan of coefficients 0..63 without restart markers, the file's own quantisation and
 * Huffman tables.  Reconstruction is libjpeg's: integer dequantisation, the "islow" inverse DCT, fancy (triangle) chroma
 * up-sampling, the 16-bit fixed-point colour tables.  Integer arithmetic throughout: the bytes do not depend on the
 * device, the batch or the run.
 *
 * A scan without restart markers is one serial Huffman chain.  It is cut into subsequences of 128 bytes, one thread each,
 * and decoded by the self-synchronising scheme: every thread decodes its subsequence from a blind state, then again and
 * again from the end state its predecessor reached, until nothing changes.  A fixed point of that chain is the sequential
 * decoder's answer; whether it was reached is checked, not assumed (status bit 0).  Pictures whose code stream does not
 * synchronise (noise at quality 100) report that bit and are the caller's to decode otherwise.
 *
 * Conventions (those of t2v_jpeg.h)
 *   - every pointer but `stream` is a DEVICE pointer the caller allocated and keeps alive until the stream has drained;
 *   - asynchronous: the work is enqueued on `stream` (a hipStream_t; NULL = the default stream); nothing synchronises and
 *     nothing allocates.  One call is a fixed sequence of launches that depends on the arguments alone, never on the
 *     content;
 *   - every call returns T2V_JPEGDEC_OK (0) or a negative status; t2v_jpegdec_last_error() returns a thread-local
 *     message.  A refused call (T2V_JPEGDEC_ERR_INVALID) has launched nothing.
 *
 * ABI note: version 1 is the six entry points below.  A new entry point or a new status bit raises the version; the
 * binding (text2video_amd/_jpegdeclib.py) refuses a library of another version.
 */
#ifndef T2V_JPEG_DECODE_H_
#define T2V_JPEG_DECODE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_JPEGDEC_ABI_VERSION 1

typedef enum {
    T2V_JPEGDEC_OK = 0,
    T2V_JPEGDEC_ERR_INVALID = -1, /* bad argument / unsupported geometry */
    T2V_JPEGDEC_ERR_HIP = -2      /* a HIP runtime call failed */
} t2v_jpegdec_status;

enum { T2V_JPEGDEC_MIN_DIM = 8, T2V_JPEGDEC_MAX_DIM = 2048, T2V_JPEGDEC_MAX_IMAGES = 1024 };

/* bits of the per-image status word decode_u8 writes */
enum {
    T2V_JPEGDEC_NOT_CONVERGED = 1, /* the synchronisation did not reach its fixed point */
    T2V_JPEGDEC_CORRUPT = 2        /* an invalid code, a stream that ends before the last block, a wrong block count */
};

/* T2V_JPEGDEC_ABI_VERSION of the library that was loaded. */
int t2v_jpegdec_abi_version(void);

/* Message of the last call on this thread that returned a negative status ("" before the first). */
const char* t2v_jpegdec_last_error(void);

/* 1 if t2v_jpegdec_decode_u8 takes H x W images of this sampling, else 0.  `sampling` is Pillow's `subsampling` number:
 * 0 = 4:4:4, 1 = 4:2:2 (Y 2x1), 2 = 4:2:0 (Y 2x2); T2V_JPEGDEC_MIN_DIM <= H, W <= T2V_JPEGDEC_MAX_DIM.  (The minimum is 8
 * because libjpeg replaces fancy up-sampling by replication once a down-sampled row has 2 samples or fewer.) */
int t2v_jpegdec_supported(int H, int W, int sampling);

/* Bytes of one image's table blob (3968).  Layout, little-endian:
 *      0  uint16 quant[3][64]   the quantisation table of component 0, 1, 2 (Y, Cb, Cr) in natural (row-major) order
 *    384  four Huffman decode tables of 896 bytes: DC of Y, AC of Y, DC of Cb / Cr, AC of Cb / Cr.  Each:
 *           0  uint16 look[256]    indexed by the next 8 bits: (code length << 8) | symbol for codes of at most 8 bits,
 *                                  0 where the code is longer
 *         512  int32  maxcode[16]  the largest code of length l at [l - 1], -1 where there is none
 *         576  int32  valoff[16]   a length-l code's symbol is vals[code + valoff[l - 1]]
 *         640  uint8  vals[256]    the symbols in code order (HUFFVAL), zero-filled
 * The kernels bound every index they take from a blob, so a wrong blob yields wrong pixels or a status, nothing else. */
size_t t2v_jpegdec_table_bytes(void);

/* Bytes of device workspace t2v_jpegdec_decode_u8 needs (0: a call it refuses).  The workspace holds two copies of the
 * subsequence end states (uint64 [nimg][ceil(scan_capacity / 128)]), the subsequences' first block ordinals, the
 * coefficients (int16 [nimg][blocks][64], natural order, blocks in coding order) and the three component planes at their
 * block-grid size; its content is scratch, a multiple of 256 bytes, and the pointer passed must be 256-byte aligned. */
size_t t2v_jpegdec_workspace_bytes(int H, int W, int sampling, int nimg, size_t scan_capacity);

/* Decode nimg files of one geometry and sampling.
 *   scans          uint8 [nimg][scan_capacity], 16-byte aligned: image i's entropy-coded bytes -- everything between the SOS
 *                  header and EOI, stuffed FF 00 pairs as in the file -- start at scans + i * scan_capacity
 *   scan_capacity  bytes per slot, a multiple of 16, 16 .. 2^28
 *   scan_lengths   uint32 [nimg]: the byte length of every scan.  Bytes from there on count as absent; a length beyond
 *                  scan_capacity is taken as scan_capacity and reported as corrupt
 *   tables         uint8 [nimg][t2v_jpegdec_table_bytes()], 4-byte aligned: every image's own table blob
 *   workspace      t2v_jpegdec_workspace_bytes(...) bytes, 256-byte aligned
 *   dst            uint8 [nimg][H][W][dst_cs], dst_cs 3 or 4: R, G, B in channels 0..2; channel 3 is written as 0
 *   status         uint32 [nimg]: 0 = decoded; T2V_JPEGDEC_NOT_CONVERGED and / or T2V_JPEGDEC_CORRUPT otherwise
 * An image with a non-zero status leaves unspecified bytes in its own dst slot and nowhere else; the other images of the
 * batch are unaffected.  No read goes past scan_capacity bytes of an image's slot.  One memset and eight launches,
 * whatever the content. */
int t2v_jpegdec_decode_u8(void* stream, const uint8_t* scans, size_t scan_capacity, const uint32_t* scan_lengths,
                          const uint8_t* tables, int H, int W, int sampling, int nimg, void* workspace, uint8_t* dst, int dst_cs,
                          uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* T2V_JPEG_DECODE_H_ */

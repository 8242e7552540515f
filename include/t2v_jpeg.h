/*
 * t2v_jpeg.h -- C ABI of libt2v_jpeg.so: a baseline JPEG encoder for the MI355X (gfx950) that writes, byte for byte, the
 * entropy-coded scan libjpeg / Pillow's Image.save(format="JPEG", quality=Q) writes for an RGB image.
 *
 * The library stands alone (nothing of libt2v_hip.so, no context object): raw device pointers and a hipStream_t in,
 * bytes out.  The part of the file that does not depend on the pixels -- SOI, APP0, DQT, SOF0, DHT, SOS in front of the
 * scan and EOI behind it -- is 623 + 2 bytes the host writes (text2video_amd/jpeg.py: header(), file_bytes()).
 *
 * Format (DESIGN.md section 4.10 has the rules in full): baseline sequential JFIF, 8 bit, Y 2x2 / Cb 1x1 / Cr 1x1, one
 * interleaved scan without restart markers, the ITU-T T.81 Annex K quantisation tables scaled by the IJG quality rule,
 * the Annex K Huffman tables, libjpeg's integer colour conversion, h2v2 down-sampling with the alternating bias and the
 * "islow" forward DCT.  Integer arithmetic throughout: the bytes do not depend on the device, the batch or the run.
 *
 * Conventions (those of t2v.h)
 *   - every pointer but `stream` is a DEVICE pointer the caller allocated and keeps alive until the stream has drained;
 *   - asynchronous: the work is enqueued on `stream` (a hipStream_t; NULL = the default stream); nothing synchronises and
 *     nothing allocates.  One call is a fixed sequence of launches that depends on (H, W, nimg) alone, never on the
 *     content;
 *   - every call returns T2V_JPEG_OK (0) or a negative status; t2v_jpeg_last_error() returns a thread-local message.
 *     A refused call (T2V_JPEG_ERR_INVALID / _WORKSPACE) has launched nothing.
 */
#ifndef T2V_JPEG_H_
#define T2V_JPEG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_JPEG_ABI_VERSION 1

typedef enum {
    T2V_JPEG_OK = 0,
    T2V_JPEG_ERR_INVALID = -1,   /* bad argument / unsupported geometry */
    T2V_JPEG_ERR_HIP = -2,       /* a HIP runtime call failed */
    T2V_JPEG_ERR_WORKSPACE = -3  /* reserved: the caller sizes the workspace with t2v_jpeg_workspace_bytes() */
} t2v_jpeg_status;

enum { T2V_JPEG_MIN_DIM = 8, T2V_JPEG_MAX_DIM = 2048, T2V_JPEG_MAX_IMAGES = 1024 };

/* T2V_JPEG_ABI_VERSION of the library that was loaded. */
int t2v_jpeg_abi_version(void);

/* Message of the last call on this thread that returned a negative status ("" before the first). */
const char* t2v_jpeg_last_error(void);

/* 1 if t2v_jpeg_encode_u8 takes H x W images (T2V_JPEG_MIN_DIM <= H, W <= T2V_JPEG_MAX_DIM), else 0.  Every other entry
 * refuses a geometry this one refuses. */
int t2v_jpeg_supported(int H, int W);

/* Bytes of device workspace t2v_jpeg_encode_u8 needs for nimg H x W images (0: a call it refuses).  The workspace holds
 * the quantised coefficients (int16 [nimg][mcus][6][64], zigzag order), the per-block bit counts and bit offsets, the
 * packed bit stream before byte stuffing and the per-chunk 0xFF counts; its content is scratch, a multiple of 256 bytes,
 * and the pointer passed must be 256-byte aligned. */
size_t t2v_jpeg_workspace_bytes(int H, int W, int nimg);

/* A number of bytes no scan of an H x W image can exceed (0: a geometry t2v_jpeg_supported refuses).
 * With B = 6 ceil(W/16) ceil(H/16) coded blocks (dummy blocks included):
 *   - a block's DC symbol is at most an 11-bit code (chroma category 11) plus 11 value bits = 22 bits;
 *   - each of its 63 AC coefficients is at most a 16-bit code plus 10 value bits = 26 bits (a zero costs less: it is
 *     part of a run, of a ZRL worth 16 zeros in 11 bits, or of the EOB); an EOB is only sent when coefficient 63 is
 *     zero, i.e. in place of something longer;
 *   so a block is at most 22 + 63 * 26 = 1660 bits = 207.5 bytes, the stream before stuffing at most 208 B bytes with its
 *   padding, and since stuffing at most doubles it, the scan at most 416 B bytes. */
size_t t2v_jpeg_scan_capacity(int H, int W);

/* Copy one uint8 HWC image into another with other channel strides, each of the first three channels through `lut` (a
 * HOST array of 256 bytes, read before the call returns; NULL = identity): how a 3-channel image, or one whose values
 * still need a byte-to-byte map, gets into a batch for t2v_jpeg_encode_u8.  dst channels >= 3 are written as 0.
 * src_cs, dst_cs in {3, 4}; npix = H * W >= 1.  One launch. */
int t2v_jpeg_stage_u8(void* stream, const uint8_t* src, int src_cs, uint8_t* dst, int dst_cs, long npix, const uint8_t* lut);

/* Encode nimg images of one geometry.
 *   src            uint8 [nimg][H][W][src_cs], src_cs 3 or 4: R, G, B in channels 0..2 (channel 3 is ignored)
 *   quality        1..100, the IJG quality (Pillow's `quality`)
 *   workspace      t2v_jpeg_workspace_bytes(H, W, nimg) bytes, 256-byte aligned
 *   out            uint8 [nimg][out_capacity]: image i's scan starts at out + i * out_capacity
 *   out_capacity   bytes per image, >= 1; t2v_jpeg_scan_capacity(H, W) always suffices
 *   lengths        uint32 [nimg]: the byte length of every scan (final 1-bit padding and stuffed 0x00 bytes included,
 *                  no EOI)
 * Writes never pass out_capacity per image: a scan longer than that is reported through lengths[i] > out_capacity, its
 * first out_capacity bytes are valid and nothing beyond them is touched.  Bytes of `out` between lengths[i] and
 * out_capacity keep their values.  Seven launches and one memset, whatever the content. */
int t2v_jpeg_encode_u8(void* stream, const uint8_t* src, int src_cs, int H, int W, int nimg, int quality, void* workspace,
                       uint8_t* out, size_t out_capacity, uint32_t* lengths);

#ifdef __cplusplus
}
#endif
#endif /* T2V_JPEG_H_ */

/*
 * t2v_png.h -- C ABI of libt2v_png.so: a lossless PNG writer for the MI355X (gfx950).  uint8 RGB images on the device in,
 * complete PNG files (signature ... IEND) on the device out; every standard PNG reader decodes them to the input pixels.
 *
 * The library stands alone (nothing of libt2v_hip.so, no context object): raw device pointers and a hipStream_t in,
 * bytes out.
 *
 * Format (DESIGN.md section 4.12 has the rules in full; tests/png_reference.py is their definition): signature, IHDR
 * (8-bit truecolour, no interlace), one IDAT, IEND, no ancillary chunk.  zlib header 78 01.  Every row gets the filter
 * type with the smallest sum of absolute (signed-byte) residuals, the lowest type on a tie.  Every band of 8 rows is one
 * dynamic-Huffman Deflate block; its tokens are literals and distance-1 matches over maximal runs of equal bytes; its
 * code lengths come from a deterministic minimum-redundancy construction limited to 15 (7 for the code-length alphabet).
 * Integer arithmetic throughout: the bytes do not depend on the device, the batch or the run.
 *
 * Conventions (those of t2v_jpeg.h)
 *   - every pointer but `stream` is a DEVICE pointer the caller allocated and keeps alive until the stream has drained;
 *   - asynchronous: the work is enqueued on `stream` (a hipStream_t; NULL = the default stream); nothing synchronises and
 *     nothing allocates.  One call is a fixed sequence of launches that depends on (H, W, nimg) alone, never on the
 *     content;
 *   - every call returns T2V_PNG_OK (0) or a negative status; t2v_png_last_error() returns a thread-local message.
 *     A refused call (T2V_PNG_ERR_INVALID / _WORKSPACE) has launched nothing.
 */
#ifndef T2V_PNG_H_
#define T2V_PNG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_PNG_ABI_VERSION 1

typedef enum {
    T2V_PNG_OK = 0,
    T2V_PNG_ERR_INVALID = -1,   /* bad argument / unsupported geometry */
    T2V_PNG_ERR_HIP = -2,       /* a HIP runtime call failed */
    T2V_PNG_ERR_WORKSPACE = -3  /* reserved: the caller sizes the workspace with t2v_png_workspace_bytes() */
} t2v_png_status;

enum { T2V_PNG_MIN_DIM = 1, T2V_PNG_MAX_DIM = 2048, T2V_PNG_MAX_IMAGES = 1024, T2V_PNG_BAND_ROWS = 8 };

/* T2V_PNG_ABI_VERSION of the library that was loaded. */
int t2v_png_abi_version(void);

/* Message of the last call on this thread that returned a negative status ("" before the first). */
const char* t2v_png_last_error(void);

/* 1 if t2v_png_encode_u8 takes H x W images (T2V_PNG_MIN_DIM <= H, W <= T2V_PNG_MAX_DIM; 1 x 1 is an image), else 0.
 * Every other entry refuses a geometry this one refuses. */
int t2v_png_supported(int H, int W);

/* Bytes of device workspace t2v_png_encode_u8 needs for nimg H x W images (0: a call it refuses).  The workspace holds
 * the filtered rows, per band the histogram, the code table and the packed block header, the per-row Adler-32 partial
 * sums, the bit offsets and the packed Deflate stream; its content is scratch, a multiple of 256 bytes, and the pointer
 * passed must be 256-byte aligned. */
size_t t2v_png_workspace_bytes(int H, int W, int nimg);

/* A number of bytes no file of an H x W image can exceed (0: a geometry t2v_png_supported refuses).
 * With B = ceil(H / 8) bands and N = H (1 + 3 W) filtered bytes:
 *   - a block header is 3 + 5 + 5 + 4 bits, at most 19 x 3 bits of code-length code lengths and at most 287 coded lengths
 *     (286 literal/length codes and one distance code).  A coded length costs at most 7 bits, the limit of its alphabet;
 *     a repeat symbol costs at most 7 + 7 bits and stands for at least 3 lengths, so it never costs more than the
 *     lengths it replaces.  A header is therefore at most 17 + 57 + 287 x 7 = 2083 bits, the largest there is;
 *   - a literal is at most 15 bits, the code limit; a match is at most 15 + 5 extra bits + the 1-bit distance code = 21
 *     bits and stands for at least 3 bytes, so no filtered byte costs more than 15 bits;
 *   - the end-of-block symbol is at most 15 bits;
 *   so the Deflate stream is at most B (2083 + 15) + 15 N bits, and the file that many bytes (rounded up) + 63: the
 *   signature (8), IHDR (25), the IDAT's length, type and CRC (12), the zlib header (2), Adler-32 (4) and IEND (12). */
size_t t2v_png_file_capacity(int H, int W);

/* Encode nimg images of one geometry.
 *   src            uint8 [nimg][H][W][src_cs], src_cs 3 or 4: R, G, B in channels 0..2 (channel 3 is ignored whatever it
 *                  holds)
 *   workspace      t2v_png_workspace_bytes(H, W, nimg) bytes, 256-byte aligned
 *   out            uint8 [nimg][out_capacity]: image i's complete file starts at out + i * out_capacity
 *   out_capacity   bytes per image, >= 1; t2v_png_file_capacity(H, W) always suffices
 *   lengths        uint32 [nimg]: the byte length of every file
 * Writes never pass out_capacity per image: a file longer than that is reported through lengths[i] > out_capacity, its
 * first out_capacity bytes are valid and nothing beyond them is touched.  Bytes of `out` between lengths[i] and
 * out_capacity keep their values.  Seven launches and one memset, whatever the content. */
int t2v_png_encode_u8(void* stream, const uint8_t* src, int src_cs, int H, int W, int nimg, void* workspace, uint8_t* out,
                      size_t out_capacity, uint32_t* lengths);

#ifdef __cplusplus
}
#endif
#endif /* T2V_PNG_H_ */

/*
 * hdlz_png_write.h -- extension of hdlz_png.h: PNG files WRITTEN on the device.  hdlz_png.h reads the container; this header closes the
 * pair, as hdlz_zip_write.h did for ZIP.  Three steps: hdlz_png_filter_ws runs the PNG predictor forwards over a batch of images (the
 * filter of every row chosen on the device), the caller's ONE hdlz_compress_batch_bits (hdlz_join.h) deflates the filtered streams of
 * all images, and hdlz_png_write_ws frames every image's blocks as a PNG file that libpng, Pillow and hdlz_png_index_ws read.
 * Additive: HDLZ_VERSION and every declaration of the headers this one includes stay as they are, and their conventions (device
 * pointers, ownership, extents, "writes" / "reads", return values) hold here too.  All words of the format are big-endian.
 *
 * THE INPUT.  n images; image i is a 24-byte hdlz_png_spec on the device.  Its samples lie at d_pix + pix_off in exactly the layout
 * HDLZ_PNG_EXPAND delivers: C-order (height, width, channels), uint8 for depth 8, LITTLE-endian uint16 for depth 16, channels =
 * 1, 3, 2, 4 for colour 0, 2, 4, 6 -- the 8 pairs (colour 0 / 2 / 4 / 6) x (depth 8 / 16).  row_bytes = width * channels * depth / 8,
 * raw_len = height * (row_bytes + 1): the filtered stream, per row a filter byte and row_bytes filtered bytes.
 *
 * THE FILTER RULE, a serial text (tests/png_write_ref.py states it in Python).  The bytes of a row are its scanline bytes: 16-bit
 * samples big-endian.  bpp = channels * depth / 8, and for the byte x at position p of a row: a = the byte at p - bpp of the same row (0
 * for p < bpp), b = the byte at p of the row above (0 above the first row), c = the byte at p - bpp of the row above (0 for p < bpp or
 * above the first row) -- exactly hdlz_png.h's predictors, on the unfiltered bytes.  The filtered byte is y = x - prediction mod 256:
 *   f = 0: 0;  1: a;  2: b;  3: (a + b) >> 1, the sum in 9 bits;  4: paeth, where p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|
 *   and paeth = a if pa <= pb and pa <= pc, else b if pb <= pc, else c.
 * mode 0 .. 4: that filter for every row.  mode 5 = HDLZ_PNG_FILTER_ADAPTIVE: for every row and every f in 0 .. 4, S_f = the sum over the
 * row's bytes of (y < 128 ? y : 256 - y); the row takes the f with the smallest S_f, a tie goes to the lowest f (libpng's order).  The
 * sums are exact (64 bits: a row can exceed 32 bits of sum).
 * Per-image refusals of the filter, the first that applies (a failed image counts 0 bytes and 0 rows and does not stop the others):
 *   width or height 0 or >= 2^31                                   HDLZ_E_BAD_HEADER
 *   (colour, depth) not one of the 8 pairs, or a reserved byte set HDLZ_E_BAD_HEADER
 *   raw_len > 2^32 - 512                                           HDLZ_E_OUT_CAPACITY
 *   the height * row_bytes pixel bytes not inside d_pix[0 .. pix_len)     HDLZ_E_BAD_PARAM
 *   raw_off[i] + raw_len > raw_cap (raw_off as below)              HDLZ_E_OUT_CAPACITY (the image still counts in raw_off: a call with
 *                                                                  raw_cap = 0 sizes the streams)
 * The streams of the images are PACKED one behind the other: raw_off = the exclusive scan of raw_len over the images that pass the
 * first four lines, raw_off[n] the total -- so one ragged hdlz_compress_batch_bits takes the blocks of all images.
 *
 * THE BLOCKS are the caller's: per image chain.plan_blocks of hdl_deflate_amd (full blocks of `block` bytes, a tail under 5 bytes
 * avoided), computed on the host from the dimensions alone; an image with raw_len < 5 gets no blocks.  Image i owns the blocks
 * [F_i, F_{i+1}), F = d_blk_first (n + 1 words), and block b of it holds the in_off[b + 1] - in_off[b] bytes of its stream that start at
 * byte in_off[b] - in_off[F_i]: only DIFFERENCES of d_in_off are used.  A batch of blocks has no gaps, so the packed streams are the
 * compress call's input as they stand unless an image without blocks lies between two that have some: then the caller compresses
 * the blocked streams from a buffer of their own (Engine.encode_png copies them there).
 *
 * THE FILE RULE, a serial text; every file equals it for every input (tests/png_write_ref.py).  Image i's file is
 *   89 50 4E 47 0D 0A 1A 0A | IHDR (13 bytes: width, height, depth, colour, 0, 0, 0) | the zlib stream Z cut into IDAT chunks of idat_len
 *   data bytes, the last one shorter and never empty | IEND
 * every chunk as length, type, data and the true CRC-32 of type + data.
 *   Z with blocks:      78 9C, the members M_b of hdlz_join.h for b in [F_i, F_{i+1}), 03 00, Adler-32 of the filtered stream big-endian.
 *                       The Adler-32 is combined from the rows' trailer words and the block lengths, as the join does: no stream byte
 *                       is read again.
 *   Z without blocks:   78 9C 01 LEN NLEN (16 bits each, little-endian), the stream's raw_len < 5 bytes, Adler-32: one final stored block.
 *   zlen = |Z|, nidat = ceil(zlen / idat_len), file_len = 33 + zlen + 12 nidat + 12; stream byte s lies at 41 + s + 12 (s / idat_len) of
 *   the file.  The files are PACKED: file_off = the exclusive scan of file_len, a failed image counts 0.
 * Failing images of the writer, the first cause that applies wins:
 *   the spec: the first three lines of the filter's list            that status
 *   d_filter_status[i] (when given) is not HDLZ_OK                  that status
 *   F_i > F_{i+1} or F_{i+1} > nblocks                              HDLZ_E_BAD_PARAM
 *   a block of the image whose status is not HDLZ_OK                the numerically largest such status
 *   a row whose length, end bit and row_pitch contradict each other (hdlz_zip_write.h step 1), or a block of negative length   HDLZ_E_BAD_PARAM
 *   the blocks' lengths do not sum to raw_len; no blocks and raw_len >= 5; no blocks and d_raw NULL; raw_off[i + 1] - raw_off[i] is
 *   not raw_len                                                     HDLZ_E_BAD_PARAM
 * The record's status, in order of precedence: the largest status of any failed image, first_bad = the lowest failed image (the sound
 * images are still written); HDLZ_E_OUT_CAPACITY when total_len > file_cap -- the true lengths and offsets are still reported and no
 * byte of d_file is written: file_cap = 0 is the sizing call --; otherwise HDLZ_OK.  first_bad is all ones when no image failed.
 * d_images, when given: for a sound image the record hdlz_png_index_ws would write for its file under `flags` and `out_align` over
 * (d_file, d_file_off, d_file_len) -- the writer hands back a ready index, also when the files did not fit; an image whose stream
 * exceeds the reader's 2^28 - 7 bytes is WRITTEN and cannot be read back here: its record is the index's, HDLZ_E_OUT_CAPACITY.  A
 * failed image: every field is 0 but file_off, the three offsets and the status, which is the image's own.
 *
 * Not there: palette images and depths below 8; Adam7; ancillary chunks (tRNS, gAMA, text, ...); dynamic-tree or stored-when-shorter
 * blocks for incompressible images (a noisy image grows by an eighth); a search over filters by compressed size; APNG; writing straight
 * into a ZIP in one call (Engine.encode_png, then Engine.compress_zip with store set over the files does it).
 */
#ifndef HDLZ_PNG_WRITE_H
#define HDLZ_PNG_WRITE_H
#include "hdlz_png.h"
#include "hdlz_join.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDLZ_PNG_FILTER_ADAPTIVE 5u
/* what the filter kernel branches on (tests read them): a wave takes HDLZ_PNGW_BAND rows of one image; a wave step covers
 * HDLZ_PNGW_STEP bytes of a row (64 lanes x 16 bytes); in adaptive mode a row of up to HDLZ_PNGW_ROW_REG_MAX bytes stays in registers
 * between the sums and the chosen filter's bytes -- a wider row is loaded a second time, right behind the first, while the L2 holds it. */
#define HDLZ_PNGW_BAND 8u
#define HDLZ_PNGW_STEP 1024u
#define HDLZ_PNGW_ROW_REG_MAX 4096u

typedef struct hdlz_png_spec {      /* 24 bytes */
    uint64_t pix_off;               /* where the image's samples start in d_pix */
    uint32_t width, height;
    uint8_t depth, colour, reserved[6];      /* reserved: 0 */
} hdlz_png_spec;

typedef struct hdlz_png_write_result {      /* 24 bytes */
    uint64_t total_len;             /* the sum of the file lengths, failed images counting 0 */
    uint64_t first_bad;             /* the lowest failed image; all ones when none failed */
    uint32_t status, reserved;      /* reserved: 0 */
} hdlz_png_write_result;

/* scratch of hdlz_png_filter_ws: 0 for n = 0 or n >= 2^31, else 2 r256(8 (n + 1)), r256 = rounded up to 256 (per image where its rows
 * and its bands start). */
size_t hdlz_png_filter_work_bytes(uint64_t n);

/*
 * Pixels -> the filtered streams: THE FILTER RULE above.  The host reads nothing inside the call.  Two launches: k_pngw_plan, ONE
 * workgroup over the images (the checks, the scans of raw_len, rows and bands), and k_pngw_filter, the hot path: a wave per band of
 * HDLZ_PNGW_BAND rows of one image, found by a search in the plan; lanes run along the row with 16-byte loads, the row above is loaded
 * the same way, the left neighbours come from the neighbouring lane's registers, 16-bit samples are swapped in registers, the five
 * sums are kept per lane and reduced across the wave, and the output -- rows of pitch row_bytes + 1, so at every alignment -- is staged
 * through LDS and stored in whole 16-byte pieces to aligned addresses, heads and tails as single bytes.
 *   total_rows    what the host knows of the sum of the heights: sizes the grid of k_pngw_filter and d_row_filter and nothing else --
 *                 the waves stride when it understated the rows, and any value gives the same streams
 *   d_row_filter  nullable: total_rows bytes, WRITTEN: the filter of row r of image i at row_base[i] + r, row_base = the exclusive scan
 *                 of the heights of the images that passed; rows at or behind total_rows are not reported
 *   d_status      n words, WRITTEN: every image's status
 *   d_raw_off     n + 1 words, WRITTEN
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: with n > 0 any of d_specs, d_status, d_raw_off
 * NULL; d_pix NULL with pix_len > 0; d_raw NULL with raw_cap > 0; n >= 2^31; mode above 5; total_rows >= 2^40; d_work NULL or
 * work_bytes below the query; d_specs, d_raw_off or d_work not 8-byte aligned; d_status not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: of d_raw exactly the streams of the images whose status is HDLZ_OK, never a byte at or behind raw_cap; d_row_filter[0 ..
 *         min(rows, total_rows)) when given; d_status[0 .. n); d_raw_off[0 .. n]; d_work[0 .. work_bytes).
 * reads:  d_specs[0 .. n); of d_pix only the pixel bytes of images that passed the checks -- no load outside them, at any alignment.
 *         The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_png_filter_ws(const uint8_t* d_pix, uint64_t pix_len, const hdlz_png_spec* d_specs, uint64_t n, uint32_t mode, uint64_t total_rows,
                       uint8_t* d_raw, uint64_t raw_cap,
                       uint8_t* d_row_filter,       /* nullable */
                       uint32_t* d_status, uint64_t* d_raw_off, void* d_work, size_t work_bytes, void* stream);

/*
 * bytes that hold the files of n images cut into nblocks blocks of at most block_len bytes:
 *     Z + 12 (Z / idat_len) + 57 n,   Z = 15 n + nblocks (hdlz_out_bound(block_len) - 1)
 * (a member is at most hdlz_out_bound(block_len) - 1 bytes, 78 9C 03 00 and the Adler-32 or a stored stream at most 15 per image; 45
 * bytes of signature, IHDR and IEND and a last partial chunk's 12 per image.)  0 for idat_len = 0.  total_raw does not enter: it is
 * taken so that a later form of the rule (stored-when-shorter) may use it.
 */
size_t hdlz_png_write_bound(uint64_t n, uint64_t total_raw, uint64_t nblocks, uint32_t block_len, uint32_t idat_len);

/* scratch of hdlz_png_write_ws: 0 for n = 0, n >= 2^31 or nblocks >= 2^31, else
 *     5 r256(8 (nblocks + 1)) + 2 r256(8 (n + 1)) + 2 r256(4 n) + 256
 * (per block the exclusive prefixes of the member lengths, of the failure counts and of the three Adler sums; per image zlen and where
 * its chunks start; its Adler-32 and status; a summary.) */
size_t hdlz_png_write_work_bytes(uint64_t n, uint64_t nblocks);

/*
 * Write the files: THE FILE RULE above.  The host reads nothing inside the call.  Four launches: k_pngw_scan, ONE workgroup over the
 * blocks (the five prefixes; nblocks = 0: not launched); k_pngw_layout, ONE workgroup over the images (the checks, zlen from two
 * prefix words, the Adler-32, the scans, the records); k_pngw_gather, a wave per block that moves M_b to its place -- a member may
 * straddle chunk seams -- and a wave per image for the signature, IHDR, the chunk heads, 78 9C, the stream's tail and IEND; k_pngw_crc,
 * a workgroup per IHDR and IDAT chunk (crc_block, the loop hdlz_png_decode_ws checks them with), strided beyond 4096 workgroups.
 *   d_raw / d_raw_off / d_filter_status   what hdlz_png_filter_ws left; d_raw is read only for an image without blocks (NULL allowed
 *                 when there is none), d_filter_status is nullable
 *   flags / out_align   HDLZ_PNG_RAW or HDLZ_PNG_EXPAND and a power of two in [1, 256]: for the records of d_images only
 *   d_file_off, d_file_len   n words each, WRITTEN;  d_image_status (nullable): n words, WRITTEN
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; n >= 2^31; nblocks >= 2^31, or
 * nblocks > 0 with n = 0; with n > 0 any of d_specs, d_raw_off, d_blk_first, d_file_off, d_file_len NULL; with nblocks > 0 any of
 * d_in_off, d_rows, d_len, d_end_bits, d_status NULL; d_file NULL with file_cap > 0; idat_len not in [1, 2^31 - 1]; flags not
 * HDLZ_PNG_RAW or HDLZ_PNG_EXPAND; out_align not a power of two in [1, 256]; d_work NULL or work_bytes below the query; d_specs,
 * d_raw_off, d_in_off, d_end_bits, d_blk_first, d_file_off, d_file_len, d_images, d_result or d_work not 8-byte aligned; d_len,
 * d_status, d_filter_status or d_image_status not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_file[0 .. total_len) when total_len <= file_cap, else no byte of it; d_file_off, d_file_len [0 .. n); d_image_status and
 *         d_images [0 .. n) when given; the record; d_work[0 .. work_bytes).
 * reads:  d_specs[0 .. n); d_raw_off, d_blk_first [0 .. n]; d_filter_status[0 .. n) when given; d_in_off[0 .. nblocks]; d_len,
 *         d_end_bits, d_status [0 .. nblocks); of row b only the bytes [2, d_len[b]), and only when its image is written; of d_raw
 *         only the stream of an image without blocks.  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_png_write_ws(const hdlz_png_spec* d_specs, uint64_t n, const uint8_t* d_raw, const uint64_t* d_raw_off,
                      const uint32_t* d_filter_status,      /* nullable */
                      const uint64_t* d_in_off, const uint8_t* d_rows, uint64_t row_pitch, const uint32_t* d_len, const uint64_t* d_end_bits,
                      const uint32_t* d_status, uint64_t nblocks, const uint64_t* d_blk_first, uint32_t idat_len, uint32_t flags, uint32_t out_align,
                      uint8_t* d_file, uint64_t file_cap, uint64_t* d_file_off, uint64_t* d_file_len,
                      uint32_t* d_image_status,      /* nullable */
                      hdlz_png_image* d_images,      /* nullable: n records, WRITTEN */
                      hdlz_png_write_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_PNG_WRITE_H */

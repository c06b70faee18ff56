/*
 * hdlz_tiff.h -- extension of hdlz_png.h: TIFF images whose strips or tiles are zlib streams (Compression 8, "Adobe deflate", and the
 * older 32946) or plain bytes (Compression 1), the tag directory walked, every strip or tile inflated and the predictor undone on the
 * device.  A deflate TIFF is not one stream but many independent ones, a strip or tile (a CHUNK) each: all chunks of all images of a
 * call are the tasks of one launch of the wave-per-member decoder.  hdlz_png.h and the headers under it read every other deflate
 * container; this one takes up TIFF.  Additive: HDLZ_VERSION and every declaration of the headers this one includes stay as they are,
 * and their conventions (device pointers, ownership, extents, "writes" / "reads", return values) hold here too.
 *
 * INPUT of both calls: that of the PNG calls -- a flat device buffer d_files[0 .. files_len) and, per image, where its file lies in
 * it: image i is d_files[file_off[i] .. file_off[i] + file_len[i]).  The slots that hdlz_zip_inflate_ws leaves behind an aligned index
 * (out_off, usize) are a valid input as they stand: TIFFs out of a ZIP are that call, then these two.  An image is ONE directory (IFD)
 * of its file, the one d_page[i] next-IFD words behind the first (d_page NULL: the first of every file): a pyramid or a stack is read
 * by naming the same file once per page.
 *
 * THE RULE (hdlz_tiff_index_ws), a serial text per image; every record equals it for every file (tests/tiff_ref.py states it in
 * Python).  The first line that applies sets the image's status.  A failed image counts 0 in all three offset scans, does not stop the
 * others, and every field of its record but file_off, file_len, status and the three offsets is 0.  len = file_len[i], page =
 * d_page[i]; a SHORT is 2 bytes, a LONG and a "word" 4, all in the file's byte order (step 1); offsets count from the file's first byte:
 *   0  file_off + file_len > files_len, or page > 65535              HDLZ_E_BAD_PARAM (nothing of the image is loaded)
 *   1  len < 4                                                       HDLZ_E_BAD_HEADER
 *      bytes 0 .. 4 are "II*\0": little-endian; "MM\0*": big-endian; "II+\0" or "MM\0+" (BigTIFF): HDLZ_E_BAD_BTYPE; anything else, or
 *      len < 8                                                       HDLZ_E_BAD_HEADER
 *   2  the hops   o = the word at 4; for k = 0 .. page:
 *        o = 0                                                       HDLZ_E_NO_EOF (no such page)
 *        o odd or o < 8                                              HDLZ_E_BAD_HEADER
 *        o + 2 > len                                                 HDLZ_E_NO_EOF
 *        nent = the SHORT at o; nent = 0                             HDLZ_E_BAD_HEADER
 *        o + 2 + 12 nent + 4 > len                                   HDLZ_E_NO_EOF
 *        next = the word at o + 2 + 12 nent; if k < page: o = next
 *      ifd_off = o, next_ifd = next (0: the last page).  At most page + 1 <= 65536 hops: a cycle of directories cannot spin.
 *   3  the tags   entry e = 0 .. nent - 1 is the 12 bytes at o + 2 + 12 e: tag (SHORT), type (SHORT), count (LONG), a value field of 4
 *      bytes.  In file order, sorted or not; of the tags 256 257 258 259 262 273 277 278 279 284 317 322 323 324 325 339 the FIRST entry
 *      of each is TAKEN, a later one and every other tag is skipped unread.  Of a taken entry:
 *        type neither 3 (SHORT) nor 4 (LONG), or count = 0           HDLZ_E_BAD_HEADER
 *        its values are count SHORTs or LONGs: where they take at most 4 bytes, in the value field; else at the offset v the value field
 *        holds: v + their bytes > len                                HDLZ_E_NO_EOF
 *        count != 1 and the tag is none of 258 339 273 279 324 325   HDLZ_E_BAD_HEADER
 *   4  the values (a tag not taken has its default)
 *        width (256) or height (257) not taken, 0 or >= 2^31         HDLZ_E_BAD_HEADER
 *        samples (277, default 1) = 0: HDLZ_E_BAD_HEADER; above 8:   HDLZ_E_BAD_BTYPE
 *        258 (BitsPerSample) or 339 (SampleFormat) taken with a count that is not `samples`      HDLZ_E_BAD_HEADER
 *        bits = the first value of 258 (default 1), format = that of 339 (default 1)
 *        bits = 0 or above 64                                        HDLZ_E_BAD_HEADER
 *        the values of 258 differ, or those of 339, or bits is none of 8 16 32 64                HDLZ_E_BAD_BTYPE
 *        format = 0 or above 6                                       HDLZ_E_BAD_HEADER
 *        format 4 5 6 (undefined, complex), or 3 (float) below 32 bits                           HDLZ_E_BAD_BTYPE
 *        compression (259, default 1) is not 1, 8 or 32946: one of 2 .. 7 (CCITT, LZW, JPEG), 32773 (PackBits), 34712, 34925, 50000
 *        (ZSTD), 50001: HDLZ_E_BAD_BTYPE; any other                  HDLZ_E_BAD_HEADER
 *        photometric (262; not taken: FFFFFFFF) = 6 (YCbCr)          HDLZ_E_BAD_BTYPE
 *        planar (284, default 1) = 2: HDLZ_E_BAD_BTYPE; neither:     HDLZ_E_BAD_HEADER
 *        predictor (317, default 1) none of 1 2 3: HDLZ_E_BAD_HEADER; 3 with a format that is not 3      HDLZ_E_BAD_BTYPE
 *   5  the layout   TILED when 322 (TileWidth) was taken: then any of 323 324 325 not taken, or 273 or 279 taken (both layouts)
 *                                                                    HDLZ_E_BAD_HEADER
 *        tile_w = 322, tile_h = 323: 0 or >= 2^31                    HDLZ_E_BAD_HEADER
 *        the chunk arrays are 324 (offsets) and 325 (byte counts)
 *      else STRIPS: 273 or 279 not taken (neither layout), or any of 323 324 325 taken           HDLZ_E_BAD_HEADER
 *        rps = 278 (RowsPerStrip; default: height) = 0               HDLZ_E_BAD_HEADER
 *        tile_w = width, tile_h = min(rps, height); the chunk arrays are 273 and 279
 *   6  geometry   px = samples * bits / 8; across = ceil(width / tile_w), down = ceil(height / tile_h), nchunks = across * down; chunk
 *      c = ty * across + tx holds the pixels [tx tile_w, (tx + 1) tile_w) x [ty tile_h, (ty + 1) tile_h).  A tile holds tile_h rows of
 *      tile_w pixels whatever of it lies outside the image; a strip only the rows inside it: every chunk decodes to full = tile_w *
 *      tile_h * px bytes, but the last strip to last = (height - (down - 1) tile_h) * width * px (tiles: last = full).
 *        nchunks >= 2^31, full > 2^32 - 512, or width * height * px > 2^62                       HDLZ_E_OUT_CAPACITY
 *        (the decoders' limits, the numbers hdlz_zip.h states; no product of the check leaves 64 bits)
 *        the count of either chunk array is not nchunks              HDLZ_E_BAD_HEADER
 *      raw_len = (nchunks - 1) full + last; out_len = height * width * px.  The byte counts and offsets of the chunks themselves are
 *      not read here (the index follows an image's tags, one dependent load a hop): hdlz_tiff_decode_ws reads and checks them.
 *   7  offsets  chunk_off, raw_off, out_off: the exclusive scans over the images of nchunks, of (nchunks - 1) r16(full) + r16(last)
 *        -- every chunk's decoded bytes rounded up to 16 --, and of out_len rounded up to out_align (a power of two from 1 to 256); a
 *        failed image counts 0.  total_chunks and total_raw are the scans' ends; total_out = out_off[last] + out_len[last], the end
 *        of the last slot (0 without images).
 *   8  capacity n > image_cap: the record's status is HDLZ_E_OUT_CAPACITY -- the totals are still the true ones and only
 *        d_images[0 .. image_cap) is written: a call with image_cap = 0 (and d_images NULL) is the sizing call.  Else the record's status
 *        is HDLZ_OK: the statuses of the images stand in their records only.
 *
 * THE PIXELS.  The slot holds C-order (height, width, samples) in LITTLE-endian samples of bits / 8 bytes, whatever the file's byte
 * order: uint for format 1, two's complement for 2, IEEE for 3.  A chunk's decoded bytes are its rows, tile_w * px bytes each:
 *   predictor 1: the samples, in the file's byte order.
 *   predictor 2: words of bits / 8 bytes in the file's byte order (floats too: the integer words); within a chunk row, sample s of pixel
 *                x is the stored word plus sample s of pixel x - 1, mod 2^bits.  Nothing carries across rows or chunks.
 *   predictor 3: a chunk row of tile_w * samples floats is stored as bits / 8 byte PLANES of tile_w * samples bytes, the most
 *                significant bytes first whatever the file's byte order; over the whole row of tile_w * px bytes, byte i is the stored
 *                byte plus byte i - samples, mod 256 (the sums run on across the planes' borders).
 * The predictor is undone whatever the compression.  Tile pixels at x >= width or y >= height are decoded and dropped.  The
 * photometric value is reported, not interpreted: palette images come back as indices, MinIsWhite is not inverted.
 *
 * Not there: BigTIFF (HDLZ_E_BAD_BTYPE); LZW, PackBits, JPEG, ZSTD and every other compression; planar configuration 2; samples below 8
 * bits or of unequal widths; YCbCr; any interpretation of the photometric value, of a palette, of the orientation or of extra samples;
 * several pages in one record (one record per page: d_page); GeoTIFF keys and every other tag (skipped unread); writing TIFF; a large
 * single-strip image among many in one call on the whole-GPU route (the caller gives it a call of its own: Engine.decode_tiff
 * decides); chunks that overlap or share bytes are read as they stand, each for itself.
 */
#ifndef HDLZ_TIFF_H
#define HDLZ_TIFF_H
#include "hdlz_png.h"

#ifdef __cplusplus
extern "C" {
#endif

/* an image of ONE deflate chunk of at least this many compressed bytes is worth a call of its own (count == 1, chunk_cap == 1: the
 * whole-GPU route); everything else is read together, a wave a chunk.  HDLZ_PNG_LARGE_MIN's number, not measured again for TIFF. */
#define HDLZ_TIFF_LARGE_MIN 16384u

typedef struct hdlz_tiff_image {    /* 136 bytes */
    uint64_t file_off, file_len;    /* the caller's words */
    uint64_t ifd_off, next_ifd;     /* the directory read, from the file's first byte -- as every offset here; the word behind it (0: the last page) */
    uint64_t off_arr, cnt_arr;      /* where the values of the two chunk arrays stand (one value: inside the entry) */
    uint64_t raw_len, out_len;
    uint64_t chunk_off, raw_off, out_off;
    uint32_t width, height, tile_w, tile_h;      /* strips: tile_w = width, tile_h = the rows of every strip but the last */
    uint32_t nchunks, compression, photometric, status;
    uint8_t off_type, cnt_type;     /* 3: SHORT, 4: LONG */
    uint8_t bits, samples, format, predictor, big_endian, tiled;
    uint8_t reserved[8];            /* 0 */
} hdlz_tiff_image;

typedef struct hdlz_tiff_index_result {
    uint64_t nimages, total_chunks, total_raw, total_out;
    uint32_t status, reserved;                    /* reserved: 0 */
} hdlz_tiff_index_result;

/* scratch of hdlz_tiff_index_ws: 0 for n = 0 or n >= 2^31, else 256 + r256(24 n), r256 = rounded up to 256 (three 64-bit sizes per
 * image).  It does not depend on image_cap: the totals need every image, in the sizing call too. */
size_t hdlz_tiff_index_work_bytes(uint64_t n, uint64_t image_cap);

/*
 * Index n TIFF images on the device: THE RULE above.  The host reads nothing inside the call.  Two launches: (a) a thread per image
 * follows its hops and tags (one dependent load a hop) and writes the record; (b) one workgroup scans the three sizes and writes the
 * offsets and the result record.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL, or with n > 0 any of d_files,
 * d_file_off, d_file_len NULL; d_images NULL with image_cap > 0; n >= 2^31; image_cap >= 2^31; out_align not a power of two in
 * [1, 256]; d_work NULL or work_bytes below the query; d_file_off, d_file_len, d_images, d_result or d_work not 8-byte aligned; d_page
 * not 4-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_images[0 .. min(n, image_cap)), the record, d_work[0 .. work_bytes).
 * reads:  d_file_off[0 .. n), d_file_len[0 .. n), d_page[0 .. n) when given; of d_files only bytes inside an image's file -- never a
 *         load outside d_files[0 .. files_len).  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_tiff_index_ws(const uint8_t* d_files, uint64_t files_len, const uint64_t* d_file_off, const uint64_t* d_file_len,
                       const uint32_t* d_page,          /* nullable: page 0 of every file */
                       uint64_t n, uint32_t out_align, uint64_t image_cap,
                       hdlz_tiff_image* d_images,       /* image_cap records, WRITTEN; NULL allowed with image_cap = 0 */
                       hdlz_tiff_index_result* d_result, void* d_work, size_t work_bytes, void* stream);

/*
 * scratch of hdlz_tiff_decode_ws: 0 for count = 0 or count >= 2^31, else
 *     r256(8 count) + r256(16 count + 272) + r256(24 chunk_cap) + r256(20 chunk_cap) + r256(8 (raw_bytes / 32768 + chunk_cap))
 *       + r256(raw_bytes) + D
 *     D = r256(hdlz_inflate_work_bytes(1, min(2 raw_bytes + 64, 2^28 - 1), min(raw_bytes rounded down to 4, 2^32 - 512), 0, 1)) when
 *         count == 1 and chunk_cap == 1, else 0
 * (two words per image; two scans and a summary; per chunk the decoder's view -- start, end, destination -- and five words; an
 * Adler-32 pair per 32 KiB tile of the decoded chunks; the decoded chunks; one chunk: the share of the batch call's path.)  chunk_cap:
 * at least the sum of nchunks over the range; raw_bytes: at least raw_off[last] - raw_off[first] + the last image's (nchunks - 1)
 * r16(full) + r16(last) -- for the whole index total_chunks and total_raw.
 */
size_t hdlz_tiff_decode_work_bytes(uint64_t count, uint64_t chunk_cap, uint64_t raw_bytes);

typedef struct hdlz_tiff_decode_result {
    uint64_t out_len;     /* out_off[first + count - 1] - out_off[first] + the last image's out_len; 0 unless status == HDLZ_OK */
    uint64_t first_bad;   /* lowest index (within this call's range) of an image that failed; ~0 when OK */
    uint32_t status;      /* HDLZ_OK, or the status of that image */
    uint32_t reserved;    /* 0 */
} hdlz_tiff_decode_result;

/*
 * Decode images [first, first + count) of an index: image e goes to its SLOT d_out + (out_off[e] - out_off[first]), out_len bytes, so
 * any sub-range decodes without the rest.  d_images: the records of hdlz_tiff_index_ws -- or of anyone else: every record is checked
 * again on the device before it is used, the first line that applies wins, and a refused image is not decoded:
 *     the record's status is not HDLZ_OK                                                       that status
 *     file_off + file_len > files_len                                                          HDLZ_E_BAD_PARAM
 *     width, height, tile_w or tile_h 0 or >= 2^31; tiled or big_endian above 1; strips with tile_w != width or tile_h > height;
 *     samples, bits, format, compression, photometric or predictor not what step 4 accepts; nchunks, raw_len or out_len not what step 6
 *     gives for them, or past its limits; off_type or cnt_type neither 3 nor 4; a chunk array that does not lie inside the file with
 *     its nchunks values                                                                       HDLZ_E_BAD_PARAM
 *     chunk_off, raw_off or out_off below the first image's; raw_off - raw_off[first] no multiple of 16; a slot that ends behind
 *     raw_bytes (the rounded chunks) or out_cap (out_len)                                      HDLZ_E_BAD_PARAM
 *     the range's chunks or Adler tiles do not fit the scratch the query sized (chunk_cap too small, overlapping slots)  HDLZ_E_BAD_PARAM
 * THE STEPS:
 *   (a) plan     a thread per chunk of the range -- its image found by a binary search in the scan of nchunks -- reads its offset
 *                and byte count n from the two arrays, in the file's byte order and the arrays' types, and checks, the first that applies:
 *                offset + n > file_len: HDLZ_E_NO_EOF; compression 8 / 32946: n < 6 (no room for the zlib header and the Adler-32):
 *                HDLZ_E_NO_EOF; n > 2^28 - 7: HDLZ_E_OUT_CAPACITY; on the one-chunk route n > 2 raw_bytes + 64 (what that route sizes
 *                itself from; a larger raw_bytes lifts it): HDLZ_E_BAD_PARAM; compression 1: n below the chunk's decoded bytes:
 *                HDLZ_E_NO_EOF (bytes beyond them are ignored).
 *   (b) decode   the deflate chunks of all images of the range are the tasks of ONE launch of the wave-per-member decoder
 *                (k_inflate_dyn<false, true>, as hdlz_zip_inflate_ws uses it), straight out of d_files -- nothing is gathered -- into
 *                the scratch.  count == 1 and chunk_cap == 1 (a single-strip image): the path of hdlz_inflate_batch_ws over the
 *                two-word ragged index of the chunk, so a large strip is decoded by the whole GPU.  Compression 1 chunks are not
 *                decoded: step (d) reads them from the file.
 *   (c) Adler-32 of every decoded chunk, a workgroup per 32 KiB tile (the sums of hdlz_inflate_checked).
 *   (d) unpredict   k_tiff_unpredict: ONE pass over the decoded bytes -- undo the predictor, swap to little-endian, crop, store into the
 *                slot.  A wave a chunk row, 1 KiB a step, every lane 16 contiguous bytes (coalesced and lane-contiguous at once); several
 *                rows a wave where a row needs fewer than 64 lanes.  Predictor 2: a lane sums its own words per channel, the wave scans
 *                the lanes' totals per channel, a carry of `samples` words goes to the row's next step.  Predictor 3: the same scan on
 *                bytes, then the planes are interleaved into words.
 *   (e) judge    per chunk, behind the checks of (a), the first that applies: the decoder's own status; the zlib header's two bytes (the
 *                rule of hdlz_inflate_checked): HDLZ_E_BAD_HEADER; decoded length above the chunk's bytes: HDLZ_E_OUT_CAPACITY; below
 *                them: HDLZ_E_BAD_CHECKSUM; the Adler-32 behind the final block not inside the byte count: HDLZ_E_NO_EOF; Adler-32
 *                mismatch: HDLZ_E_BAD_CHECKSUM.  Bytes of a chunk BEHIND its stream's Adler-32 are accepted -- unlike hdlz_png_decode_ws,
 *                which wants the IDAT bytes used up: TIFF writers pad their chunks, and libtiff ignores what follows the stream.  An
 *                image's status is that of its lowest failed chunk; a failed image does not stop the others.
 * d_image_status (nullable): count words, WRITTEN: every image's status.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; with count > 0 any of d_files,
 * d_images NULL; d_out NULL with out_cap > 0; first + count >= 2^31; chunk_cap >= 2^31 or raw_bytes >= 2^40; d_images or d_result not
 * 8-byte aligned; d_image_status not 4-byte aligned; d_work not 256-byte aligned; with count > 0, d_work NULL or work_bytes below the
 * query.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_out inside the slots of the images that passed the checks, never a byte at or behind out_cap; d_image_status[0 .. count)
 *         when given, the record, d_work[0 .. work_bytes).
 * reads:  d_images[first .. first + count); d_files[0 .. files_len) only, and of it only bytes inside the files of the range.  The
 *         initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_tiff_decode_ws(const uint8_t* d_files, uint64_t files_len, const hdlz_tiff_image* d_images, uint64_t first, uint64_t count,
                        uint64_t chunk_cap, uint64_t raw_bytes, uint8_t* d_out, uint64_t out_cap,
                        uint32_t* d_image_status,     /* nullable */
                        hdlz_tiff_decode_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_TIFF_H */

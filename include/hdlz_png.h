/*
 * hdlz_png.h -- extension of hdlz_zip.h: PNG images of any writer, the chunks walked, the IDAT stream inflated and the scanlines
 * unfiltered (and, on request, expanded to plain samples) on the device.  A PNG is a zlib stream cut into IDAT chunks plus a per-row
 * predictor over the decoded bytes; hdlz_zip.h and the headers under it read every other deflate container, this one takes up PNG.
 * Additive: HDLZ_VERSION and every declaration of the headers this one includes stay as they are, and their conventions (device
 * pointers, ownership, extents, "writes" / "reads", return values) hold here too.  All words of the format are big-endian.
 *
 * INPUT of both calls: a flat device buffer d_files[0 .. files_len) and, per image, where its file lies in it: image i is
 * d_files[file_off[i] .. file_off[i] + file_len[i]).  Two arrays, not n + 1 offsets: the slots that hdlz_zip_inflate_ws leaves behind
 * an aligned index (out_off, usize) are a valid input as they stand -- PNGs out of a ZIP are that call, then these two.
 *
 * THE RULE (hdlz_png_index_ws), a serial text per image; every record equals it for every file (tests/png_ref.py states it in Python).
 * The first line that applies sets the image's status.  A failed image counts 0 bytes in all three offset scans, does not stop the
 * others, and every field of its record but file_off, file_len, status and the three offsets is 0.  len = file_len[i]:
 *   0  file_off + file_len > files_len                               HDLZ_E_BAD_PARAM (nothing of the image is loaded)
 *   1  len < 8, or the first 8 bytes are not 89 50 4E 47 0D 0A 1A 0A   HDLZ_E_BAD_HEADER
 *      len >= 16 and bytes 8 .. 16 are not 00 00 00 0D "IHDR"        HDLZ_E_BAD_HEADER
 *   2  the walk    p = 8; seen_idat = gap = false; nidat = zlen = 0; repeat:
 *        p + 12 > len                                                HDLZ_E_NO_EOF
 *        L = the word at p; L >= 2^31                                HDLZ_E_BAD_HEADER
 *        p + 12 + L > len                                            HDLZ_E_NO_EOF
 *        the type (bytes p + 4 .. p + 8) is
 *          IEND: stop; used = p + 12 + L.  Bytes behind it are not looked at.
 *          IHDR and p != 8                                           HDLZ_E_BAD_HEADER
 *          IDAT: gap (an IDAT behind a non-IDAT chunk that followed an IDAT)      HDLZ_E_BAD_HEADER
 *                else: the first one sets idat_off = p; nidat += 1; zlen += L; seen_idat = true
 *          any other type: if seen_idat, gap = true; then
 *            bit 5 of its first byte clear and it is not IHDR / PLTE: HDLZ_E_BAD_BTYPE (an unknown critical chunk)
 *            PLTE, no IDAT seen and no PLTE taken yet: L is 0, above 768 or no multiple of 3: HDLZ_E_BAD_HEADER; else it is TAKEN:
 *                 plte_off = p + 8, plte_n = L / 3.  (A later PLTE is skipped unread.)
 *            tRNS, no IDAT seen, colour type (byte 25) 3 and none taken yet: L > 256: HDLZ_E_BAD_HEADER; else TAKEN: trns_off = p + 8,
 *                 trns_n = L.  For other colour types it is ignored (a colour key is not applied).
 *            every other ancillary chunk is skipped unread
 *        p += 12 + L
 *      at IEND: no IDAT seen, or colour type 3 and no PLTE taken     HDLZ_E_BAD_HEADER
 *   3  IHDR (bytes 16 .. 29: width, height, depth, colour, compression, filter, interlace)
 *        width or height is 0 or >= 2^31                             HDLZ_E_BAD_HEADER
 *        (colour, depth) not one of 0:{1,2,4,8,16} 2:{8,16} 3:{1,2,4,8} 4:{8,16} 6:{8,16}, or compression or filter not 0      HDLZ_E_BAD_HEADER
 *        interlace 1 (Adam7) and flags without HDLZ_PNG_ADAM7          HDLZ_E_BAD_BTYPE ("a method this call was not asked to read")
 *        interlace above 1                                           HDLZ_E_BAD_HEADER
 *        (with HDLZ_PNG_ADAM7 interlace 1 is accepted and the record's interlace is 1)
 *   4  sizes    channels = 1, 3, 1, 2, 4 for colour 0, 2, 3, 4, 6; row_bytes = ceil(width * depth * channels / 8);
 *        raw_len = height * (row_bytes + 1); raw_len > 2^32 - 512 or zlen > 2^28 - 7: HDLZ_E_OUT_CAPACITY (the decoders' limits, the
 *        numbers hdlz_zip.h states).
 *        An INTERLACED image (interlace 1, under HDLZ_PNG_ADAM7) is seven reduced images, the passes, one behind the other in the
 *        stream; pass p = 1 .. 7 takes the pixels (x0 + i dx, y0 + j dy):   p   1  2  3  4  5  6  7
 *                                                                           x0  0  4  0  2  0  1  0
 *                                                                           y0  0  0  4  0  2  0  1
 *                                                                           dx  8  8  4  4  2  2  1
 *                                                                           dy  8  8  8  4  4  2  2
 *        pw = ceil((width - x0) / dx), 0 if width <= x0; ph the same in y; a pass with pw = 0 or ph = 0 is absent from the stream;
 *        prb = ceil(pw * depth * channels / 8); raw_len = the sum over the present passes of ph * (prb + 1), held against the same
 *        limit (no product or sum of the check leaves 64 bits).  row_bytes, out_len, channels_out and sample_bytes are those of the
 *        whole image, as below: the slot holds the DEINTERLACED image under either flag.
 *        HDLZ_PNG_RAW:    channels_out = channels, sample_bytes = 2 for depth 16 else 1, out_len = height * row_bytes
 *        HDLZ_PNG_EXPAND: channels_out = channels, but 3 for colour 3 (4 when a tRNS was taken); sample_bytes as above;
 *                         out_len = height * width * channels_out * sample_bytes
 *   5  offsets  z_off, raw_off, out_off: the exclusive scans over the images of zlen + 8 rounded up to 16, of raw_len rounded up to 16
 *        and of out_len rounded up to out_align (a power of two from 1 to 256); a failed image counts 0.  total_z and total_raw are
 *        the scans' ends; total_out = out_off[last] + out_len[last], the end of the last slot (0 without images).
 *   6  capacity n > image_cap: the record's status is HDLZ_E_OUT_CAPACITY -- the totals are still the true ones and only
 *        d_images[0 .. image_cap) is written: a call with image_cap = 0 (and d_images NULL) is the sizing call.  Else the record's status
 *        is HDLZ_OK: the statuses of the images stand in their records only.
 *
 * THE PIXELS.  The decoded stream is height rows of 1 + row_bytes bytes, a filter byte f and the filtered bytes x.  With
 * bpp = max(1, depth * channels / 8), a = the unfiltered byte bpp to the left (0 in front of the row), b = the one above (0 above the
 * first row), c = the one above a:   f = 0: x;  1: x + a;  2: x + b;  3: x + ((a + b) >> 1), the sum in 9 bits;  4: x + paeth, where
 * p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c| and paeth = a if pa <= pb and pa <= pc, else b if pb <= pc, else c; all mod 256.
 * HDLZ_PNG_RAW delivers these scanlines as PNG packs them: height * row_bytes bytes, 16-bit samples big-endian, pixels below 8 bits
 * packed from the high bit, palette images as indices.
 * HDLZ_PNG_EXPAND delivers C-order (height, width, channels_out): uint8 for depths up to 8, LITTLE-endian uint16 for depth 16; grey
 * below 8 bits scaled by bit replication (x255, x85, x17); palette images as RGB, or RGBA when a tRNS was taken: alpha is 255 for an
 * index at or past trns_n, and an index at or past plte_n is (0, 0, 0), opaque.
 * An INTERLACED image: the filter rule holds inside each pass as if the pass were an image of pw x ph -- nothing is above a pass's
 * first row, bpp is the whole image's --, and a filter byte above 4 in any pass is HDLZ_E_BAD_SYMBOL.  HDLZ_PNG_EXPAND delivers exactly
 * what the same pixels deliver non-interlaced; HDLZ_PNG_RAW delivers height * row_bytes bytes of packed scanlines, the pixels below 8
 * bits packed again from the high bit, the pad bits of a row's last byte 0.
 *
 * Not there: progressive delivery of an interlaced image (a usable image after each pass); writing interlaced files; APNG frames (acTL / fcTL / fdAT are skipped: the default image is read); tRNS colour
 * keys of grey and RGB images; gamma and colour profiles (gAMA, iCCP, sRGB, cHRM are skipped); images past the decoders' limits (step
 * 4); writing PNG (hdlz_png_write.h, the extension of this header, writes it); decoding straight out of a ZIP in one call
 * (hdlz_zip_index_ws(out_align), hdlz_zip_inflate_ws, then the two calls here over (d_out, out_off, usize) do it, nothing staged in between); several large images on the whole-GPU path in one call (the
 * caller makes one call per large image, or one call over all of them when they are many: Engine.decode_png decides; INTEGRATION.md
 * section 4); a chunk walk that guesses ahead (the index and the chunk list follow a file's chunks one dependent load a hop); the
 * CRC-32 of one very long IDAT chunk by more than one workgroup.
 */
#ifndef HDLZ_PNG_H
#define HDLZ_PNG_H
#include "hdlz_zip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDLZ_PNG_RAW    0u
#define HDLZ_PNG_EXPAND 1u
/* OR-ed into either of them, in both calls: Adam7 interlaced images are read (steps 3 and 4).  Without it both calls do, launch and
 * answer what they did before the flag existed. */
#define HDLZ_PNG_ADAM7  4u
/* an image of at least this many compressed bytes is worth a call of its own (count == 1: the whole-GPU path); below it, images are
 * read together, a wave each.  (HDLZ_ZIP_LARGE_MIN's number: INTEGRATION.md section 4.) */
#define HDLZ_PNG_LARGE_MIN 16384u

typedef struct hdlz_png_image {     /* 136 bytes */
    uint64_t file_off, file_len;    /* the caller's words */
    uint64_t idat_off;              /* the first IDAT chunk (its length word), from the file's first byte -- as every offset here */
    uint64_t zlen;                  /* the sum of the IDAT data lengths: the zlib stream */
    uint64_t plte_off, trns_off;    /* the DATA of the PLTE / tRNS taken; 0: none */
    uint64_t used;                  /* the end of IEND */
    uint64_t row_bytes, raw_len, out_len;
    uint64_t z_off, raw_off, out_off;
    uint32_t width, height, nidat, plte_n, trns_n, status;       /* plte_n: entries; trns_n: bytes */
    uint8_t depth, colour, interlace, channels_out, sample_bytes, reserved[3];      /* reserved: 0 */
} hdlz_png_image;

typedef struct hdlz_png_index_result {
    uint64_t nimages, total_z, total_raw, total_out;
    uint32_t status, reserved;                    /* reserved: 0 */
} hdlz_png_index_result;

/* scratch of hdlz_png_index_ws: 0 for n = 0 or n >= 2^31, else 256 + r256(24 n), r256 = rounded up to 256 (three 64-bit sizes per
 * image).  It does not depend on image_cap: the totals need every image, in the sizing call too. */
size_t hdlz_png_index_work_bytes(uint64_t n, uint64_t image_cap);

/*
 * Index n PNG files on the device: THE RULE above.  The host reads nothing inside the call.  Two launches: (a) a thread per image walks
 * its chunks (one dependent load a hop) and writes the record; (b) one workgroup scans the three sizes and writes the offsets and the
 * result record.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL, or with n > 0 any of d_files,
 * d_file_off, d_file_len NULL; d_images NULL with image_cap > 0; n >= 2^31; image_cap >= 2^31; flags not HDLZ_PNG_RAW or
 * HDLZ_PNG_EXPAND, with or without HDLZ_PNG_ADAM7 (0, 1, 4, 5); out_align not a power of two in [1, 256]; d_work NULL or work_bytes below the query; d_file_off, d_file_len,
 * d_images, d_result or d_work not 8-byte aligned.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_images[0 .. min(n, image_cap)), the record, d_work[0 .. work_bytes).
 * reads:  d_file_off[0 .. n), d_file_len[0 .. n); of d_files only bytes inside an image's file -- never a load outside
 *         d_files[0 .. files_len).  The initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_png_index_ws(const uint8_t* d_files, uint64_t files_len, const uint64_t* d_file_off, const uint64_t* d_file_len, uint64_t n,
                      uint32_t flags, uint32_t out_align, uint64_t image_cap,
                      hdlz_png_image* d_images,       /* image_cap records, WRITTEN; NULL allowed with image_cap = 0 */
                      hdlz_png_index_result* d_result, void* d_work, size_t work_bytes, void* stream);

/*
 * scratch of hdlz_png_decode_ws: 0 for count = 0 or count >= 2^31, else
 *     r256(32 count) + r256(56 count + 288) + r256(24 (idat_cap + 4 count)) + r256(8 (raw_bytes / 32768 + count))
 *       + r256(z_bytes) + r256(raw_bytes) + D
 *     D = r256(hdlz_inflate_work_bytes(1, min(z_bytes, 2^28 - 1), min(raw_bytes rounded down to 4, 2^32 - 512), 0, 1)) when count == 1, else 0
 * (eight 32-bit and seven 64-bit words per image and a summary; the chunk list: IHDR, PLTE, tRNS, IEND and every IDAT; an Adler-32
 * pair per 32 KiB tile of the decoded streams; the gathered zlib streams; the decoded streams; one image: the share of the batch
 * call's path.)  idat_cap: at least the sum of nidat over the range; z_bytes: at least z_off[last] - z_off[first] + (zlen[last] + 8
 * rounded up to 16); raw_bytes: the same of raw_off and raw_len rounded up to 16 -- for the whole index total_z and total_raw.
 */
size_t hdlz_png_decode_work_bytes(uint64_t count, uint64_t idat_cap, uint64_t z_bytes, uint64_t raw_bytes);

typedef struct hdlz_png_decode_result {
    uint64_t out_len;     /* out_off[first + count - 1] - out_off[first] + the last image's out_len; 0 unless status == HDLZ_OK */
    uint64_t first_bad;   /* lowest index (within this call's range) of an image that failed; ~0 when OK */
    uint32_t status;      /* HDLZ_OK, or the status of that image */
    uint32_t reserved;    /* 0 */
} hdlz_png_decode_result;

/*
 * Decode images [first, first + count) of an index: image e goes to its SLOT d_out + (out_off[e] - out_off[first]), out_len bytes, so
 * any sub-range decodes without the rest.  flags: those the index was taken with.  d_images: the records of hdlz_png_index_ws -- or of
 * anyone else: every record is checked again on the device before it is used, the first line that applies wins, and a refused image
 * is not decoded:
 *     the record's status is not HDLZ_OK                                                       that status
 *     file_off + file_len > files_len, or used > file_len                                      HDLZ_E_BAD_PARAM
 *     width, height, (colour, depth), interlace not what steps 3 and 4 accept under `flags` (interlace 1: only with HDLZ_PNG_ADAM7);
 *     channels_out, sample_bytes, row_bytes, raw_len (an interlaced image: the sum over its passes) or out_len not what step 4 gives
 *     for them under `flags`                                                                   HDLZ_E_BAD_PARAM
 *     nidat = 0 or idat_off + 12 > used; colour 3: plte_n not in [1, 256] or the PLTE taken not inside [8, used); trns_n > 256 or the
 *     tRNS taken not inside [8, used)                                                          HDLZ_E_BAD_PARAM
 *     z_off, raw_off or out_off below the first image's; raw_off - raw_off[first] no multiple of 16; a slot that ends behind z_bytes
 *     (zlen + 8), raw_bytes (raw_len) or out_cap (out_len)                                     HDLZ_E_BAD_PARAM
 *     the range's chunks, Adler tiles or scans do not fit the scratch the query sized (idat_cap too small, overlapping slots)   HDLZ_E_BAD_PARAM
 *     zlen < 6 (no room for the zlib header and the Adler-32)                                  HDLZ_E_NO_EOF
 *     the chunk list: from idat_off, nidat chunks that are not all IDAT inside [8, used), whose lengths do not sum to zlen, or no
 *     IEND behind them that ends at `used`                                                     HDLZ_E_BAD_PARAM
 * THE STEPS:
 *   (a) gather   a thread per image lists its chunks (IHDR, the PLTE and tRNS taken, every IDAT, IEND); then a workgroup per 16 KiB of
 *                every image's zlib stream copies what the list says lies there -- so a large image is gathered by the whole GPU, not
 *                chunk by chunk -- to z_off in the scratch.
 *   (b) CRC-32   of every listed chunk, type and data (contiguous in the file), a workgroup per chunk (crc_block, the loop of
 *                hdlz_crc32_batch_ws); a mismatch is HDLZ_E_BAD_CHECKSUM.
 *   (c) decode   count >= 2: the task view of the wave-per-member decoder (k_inflate_dyn<false, true>), a wave per image, as
 *                hdlz_zip_inflate_ws uses it; count == 1: the path of hdlz_inflate_batch_ws over the two-word ragged index of the
 *                gathered stream, so a large image is decoded by the whole GPU (the scratch is the library's: the alignment conditions
 *                hdlz_zip.h states for that route always hold here).  Both decode to raw_off in the scratch.
 *   (d) unfilter and expand   k_png_unfilter: a wave per SEGMENT -- a segment starts at row 0 and at the first row whose filter is 0 or 1
 *                (it does not look up) of every further 64 rows, and ends where the next one starts; rows are lanes, skewed by one pixel (the diagonal
 *                wavefront: the byte above is the neighbouring lane's of the step before), 64 rows a band, the strided rows staged
 *                through LDS with coalesced 16-byte loads and written back the same way.  8-bit grey, grey-alpha, RGB and RGBA (and
 *                every type in RAW mode) go straight into the slot; the other types are unfiltered in place and a second kernel
 *                (k_png_expand: byte swap, unpack and scale, palette look-up) writes the slot.
 *                An interlaced image takes a band per 64 rows of each present pass; the segment rule holds inside a pass (a segment
 *                starts at the pass's row 0 and never crosses a pass), every pass is unfiltered in place, and k_png_deinterlace --
 *                launched only under HDLZ_PNG_ADAM7 -- writes the slot from the seven sub-images, a thread per output element (a
 *                pixel; RAW below 8 bits: a byte of a packed row), expanding as k_png_expand does, which skips such images.
 *   (e) judge    behind the record's checks and HDLZ_E_BAD_CHECKSUM of (b), per image, the first that applies -- stricter than libpng,
 *                as the ZIP reader is than unzip: the decoder's own status; the zlib header's two bytes (the rule of
 *                hdlz_inflate_checked): HDLZ_E_BAD_HEADER; decoded length above raw_len: HDLZ_E_OUT_CAPACITY; below it:
 *                HDLZ_E_BAD_CHECKSUM; compressed bytes consumed, the Adler-32 included, not zlen: HDLZ_E_NO_EOF; Adler-32 mismatch:
 *                HDLZ_E_BAD_CHECKSUM; a filter byte above 4 in any row: HDLZ_E_BAD_SYMBOL.  The same on both routes.
 * d_image_status (nullable): count words, WRITTEN: every image's status.
 * Parameter errors (HDLZ_E_BAD_PARAM before the device is looked at), in this order: d_result NULL; with count > 0 any of d_files,
 * d_images NULL; d_out NULL with out_cap > 0; first + count >= 2^31; flags not HDLZ_PNG_RAW or HDLZ_PNG_EXPAND, with or without
 * HDLZ_PNG_ADAM7; idat_cap >= 2^40,
 * z_bytes >= 2^40 or raw_bytes >= 2^40; d_images or d_result not 8-byte aligned; d_image_status not 4-byte aligned; d_work not 256-byte
 * aligned; with count > 0, d_work NULL or work_bytes below the query.
 * Nothing is allocated; every launch is capturable; only this form exists.
 * writes: d_out inside the slots of the images that passed the checks, never a byte at or behind out_cap; d_image_status[0 .. count)
 *         when given, the record, d_work[0 .. work_bytes).
 * reads:  d_images[first .. first + count); d_files[0 .. files_len) only, and of it only bytes inside the files of the range.  The
 *         initial contents of the outputs and of d_work never reach a result.
 */
int hdlz_png_decode_ws(const uint8_t* d_files, uint64_t files_len, const hdlz_png_image* d_images, uint64_t first, uint64_t count,
                       uint32_t flags, uint64_t idat_cap, uint64_t z_bytes, uint64_t raw_bytes, uint8_t* d_out, uint64_t out_cap,
                       uint32_t* d_image_status,     /* nullable */
                       hdlz_png_decode_result* d_result, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDLZ_PNG_H */

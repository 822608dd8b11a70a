/*
 * locov_jpeg.h -- baseline JPEG decoding for the dataset mapper: the entry points of liblocov_hip.so that
 * locov_amd/_lib.py binds through JPEG_SIGNATURES (csrc/jpeg_entropy.h, csrc/jpeg.hip).  Added under ABI version 8; the
 * conventions of locov_hip.h apply (extern "C", `_host` pointers, the explicit stream, "calls only enqueue").
 *
 * locov_amd/jpeg.py is the DEFINITION of everything below, and its bytes are Pillow's (libjpeg-turbo's defaults).  Two stages:
 *
 *   host    locov_jpeg_parse reads a stream's header and says whether this decoder takes it; locov_jpeg_entropy_decode turns the
 *           scans of a batch into sparse coefficient records on up to min(16, n) threads; locov_jpeg_entropy_pack lays the records
 *           out, one after the other, in the buffer that is uploaded.  None of the three touches the GPU.
 *   device  locov_jpeg_decode: dequantisation, the "islow" inverse DCT, upsampling and the colour conversion of up to
 *           LOCOV_LABEL_MAX_IMAGES images of different sizes and layouts, in two launches.
 *
 * Supported: SOF0 / SOF1 (8-bit, Huffman), 1 component, or 3 with chroma 1x1 and luma (h, v) in {(1,1), (2,1), (2,2)}, one
 * interleaved scan, DRI / RSTn, any DHT, 0xFF00 stuffing, fill bytes in front of a marker, APPn / COM.  Everything else is
 * supported = 0 with a reason; an anomaly inside the scan is a negative per-image status.  For those the caller takes Pillow: this
 * decoder never guesses what libjpeg's recovery would do.
 *
 * The record of one image, uint32 words: block_start[nblocks + 1], then one word per non-zero QUANTISED coefficient,
 * (natural-order index << 16) | (value & 0xFFFF), DC prediction undone.  Blocks are in component-plane raster order over the
 * MCU-padded grid (component 0's plane, then 1's, then 2's: plane c is mcus_across * h_c by mcus_down * v_c blocks); block b owns
 * the words [block_start[b], block_start[b + 1]) counted from the first entry, in scan (zigzag) order.
 */
#ifndef LOCOV_JPEG_H
#define LOCOV_JPEG_H

#include "locov_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* locov_jpeg_header.reason */
#define LOCOV_JPEG_REASON_OK 0
#define LOCOV_JPEG_REASON_NOT_JPEG 1          /* no SOI */
#define LOCOV_JPEG_REASON_TRUNCATED_HEADER 2  /* the data ends before the scan */
#define LOCOV_JPEG_REASON_SOF 3               /* SOF2 and above: progressive, lossless, differential */
#define LOCOV_JPEG_REASON_ARITHMETIC 4
#define LOCOV_JPEG_REASON_PRECISION 5         /* not 8 bits */
#define LOCOV_JPEG_REASON_COMPONENTS 6        /* neither 1 nor 3 */
#define LOCOV_JPEG_REASON_RGB 7               /* Adobe transform 0, or ids 'R' 'G' 'B' without a JFIF or Adobe segment */
#define LOCOV_JPEG_REASON_SAMPLING 8
#define LOCOV_JPEG_REASON_SCANS 9             /* not one interleaved scan with Ss = 0, Se = 63, Ah = Al = 0 */
#define LOCOV_JPEG_REASON_DNL 10
#define LOCOV_JPEG_REASON_QT16 11
#define LOCOV_JPEG_REASON_MISSING_TABLE 12
#define LOCOV_JPEG_REASON_BAD_TABLE 13
#define LOCOV_JPEG_REASON_SIZE 14
#define LOCOV_JPEG_REASON_SEGMENT 15

/* per-image status of locov_jpeg_entropy_decode */
#define LOCOV_JPEG_STATUS_OK 0
#define LOCOV_JPEG_STATUS_BAD_CODE (-1)       /* a bit pattern that is no Huffman code */
#define LOCOV_JPEG_STATUS_MARKER (-2)         /* a marker inside the scan that is not the expected RSTn */
#define LOCOV_JPEG_STATUS_DATA_END (-3)       /* the data runs out inside the scan */
#define LOCOV_JPEG_STATUS_NO_EOI (-4)         /* something else than EOI behind the last MCU (a second scan included) */
#define LOCOV_JPEG_STATUS_MAGNITUDE (-5)      /* outside the magnitude guards below (per coefficient, per block, quantised DC) */
#define LOCOV_JPEG_STATUS_SPACE (-6)          /* the staging buffer is smaller than locov_jpeg_entropy_bytes says */
#define LOCOV_JPEG_STATUS_INDEX (-7)          /* a run that ends past coefficient 63 */
#define LOCOV_JPEG_STATUS_UNSUPPORTED (-8)    /* header.supported == 0 */

/* The largest dequantised magnitude the decoder takes.  With |d| <= M for every coefficient, pass 1 of the IDCT ends at
 * |ws| <= (61214 * M + 2^10) >> 11 (61214 = 7.4724 * 2^13: the largest sum of absolute weights of any value in jidctint's flow graph)
 * and every value of pass 2 stays below 61214 * |ws|max + 2^17: below 2^31 up to M = 1173, and with pass 1's results inside 16 bits
 * -- how libjpeg-turbo's SIMD code keeps them -- up to M = 1096.  8-bit pixels give at most 1024 plus half a quantisation step. */
#define LOCOV_JPEG_MAX_DEQUANTISED 1096
/* The per-block range guard.  libjpeg's C code looks the descaled pass-2 result x up in a table at (x & 1023), which wraps;
 * libjpeg-turbo's SIMD code saturates.  They agree exactly for x in [-512, 511], and only such blocks are decoded.  With W_k the
 * largest |weight| of input k in the one-dimensional pass, scaled by 2^13 (8192, 11363, 10703, 11362, 8192, 11362, 10704, 11363):
 *   |ws| <= sum_k W_k |d_kl| / 2^11 + 1,   |x| <= sum_l W_l |ws_l| / 2^18 + 1/2 <= S / 2^29 + 0.82,   S = sum_kl W_k W_l |d_kl|,
 * so S <= 510 * 2^29 keeps |x| <= 511 and every pass-1 value below 16321 (sums of two stay inside 16 bits).  A block above the
 * limit is not refused on the bound: the host runs both passes on it and takes it when every pass-1 value is within 16383 and every
 * pass-2 result within [-512, 511].  The quantised DC is also held to +-32767 whatever the quantiser.  LOCOV_JPEG_STATUS_MAGNITUDE
 * covers all three guards. */
#define LOCOV_JPEG_RANGE_SUM_LIMIT (510ll << 29)

typedef struct locov_jpeg_header {
    int32_t supported, reason;                 /* 1 / 0, LOCOV_JPEG_REASON_* */
    int32_t width, height, ncomp;
    int32_t comp_id[3], comp_h[3], comp_v[3];  /* a single component has h = v = 1 here whatever the frame header says */
    int32_t comp_tq[3], comp_td[3], comp_ta[3];
    int32_t restart_interval;
    int64_t scan_start;                        /* offset of the first entropy-coded byte */
    uint8_t qt_present[4];
    uint16_t qt[4][64];                        /* natural order */
    uint8_t dc_present[4], ac_present[4];
    uint8_t dc_counts[4][16], ac_counts[4][16];
    uint8_t dc_symbols[4][256], ac_symbols[4][256];
} locov_jpeg_header;

/* Fills *header from data_host[0 .. len).  Always LOCOV_OK unless a pointer is null (LOCOV_ERR_INVALID_ARG): what is wrong with a
 * stream is header->supported == 0 and header->reason.  Every read is bounds-checked.  No GPU. */
int locov_jpeg_parse(const void *data_host, int64_t len, locov_jpeg_header *header);

/* Staging bytes locov_jpeg_entropy_decode needs for a supported stream of `len` bytes (0 for an unsupported header): a uint32
 * start per block plus one word per coefficient the scan can hold -- at most 64 per block, and at most 4 per scan byte (a
 * non-zero coefficient costs a code bit and a magnitude bit at the least). */
int64_t locov_jpeg_entropy_bytes(const locov_jpeg_header *header, int64_t len);

/* Decodes the scans of n streams (any n >= 0) on up to min(16, n) threads.  Image i: data_host[i][0 .. lens_host[i]) with
 * headers_host[i] (from locov_jpeg_parse), into staging_host[i] of staging_bytes_host[i] >= locov_jpeg_entropy_bytes bytes (HOST
 * memory, 4-byte aligned; scan order inside).  status_host[i] receives LOCOV_JPEG_STATUS_*; record_bytes_host[i] the bytes of the
 * image's record (a multiple of 16, 0 on a negative status).  Every read of the input and write of the staging is bounds-checked;
 * nothing throws.  Returns LOCOV_OK unless a pointer is null or n < 0.  No GPU. */
int locov_jpeg_entropy_decode(const void *const *data_host, const int64_t *lens_host, const locov_jpeg_header *headers_host,
                              void *const *staging_host, const int64_t *staging_bytes_host, int n, int32_t *status_host,
                              int64_t *record_bytes_host);

/* Writes the record of image i (status OK) from its staging into records_host[i][0 .. record_bytes_host[i]) -- typically n places
 * in one pinned buffer --, in the layout at the top of this header, the tail up to the multiple of 16 zeroed.  Up to min(16, n)
 * threads.  LOCOV_OK, or LOCOV_ERR_INVALID_ARG for a null pointer, n < 0 or a record_bytes that is not what decode returned. */
int locov_jpeg_entropy_pack(const locov_jpeg_header *headers_host, const void *const *staging_host, const int64_t *record_bytes_host,
                            void *const *records_host, int n);

/* ---- the pixel pipeline (csrc/jpeg.hip) ----------------------------------------------------------------------------------------
 * One image of a locov_jpeg_decode call: where its record and quantisation tables lie in `records`, and its layout. */
typedef struct locov_jpeg_desc {
    int32_t width, height, ncomp;              /* 1 or 3 */
    int32_t hs, vs;                            /* the luma's sampling factors: (1,1), (2,1) or (2,2); chroma is 1x1 */
    int32_t reserved;
    int64_t record_offset;                     /* bytes from `records`, a multiple of 16 */
    int64_t record_bytes;                      /* what locov_jpeg_entropy_decode returned for the image */
    int64_t qt_offset;                         /* bytes from `records`, a multiple of 4: ncomp x 64 uint16, natural order */
} locov_jpeg_desc;

#define LOCOV_JPEG_RGB 0
#define LOCOV_JPEG_BGR 1
#define LOCOV_JPEG_L 2                         /* grey streams only */

/* Bytes of workspace locov_jpeg_decode needs: the MCU-padded sample planes of every image, each image on a multiple of 16.
 * -1 for a descriptor outside the limits below. */
int64_t locov_jpeg_decode_workspace_bytes(const locov_jpeg_desc *descs_host, int n_images);

/* records [record_bytes] (DEVICE, 16-byte aligned) -> outs_host[i]: DEVICE uint8 [height, width, 3] in R, G, B or B, G, R order
 * (format LOCOV_JPEG_RGB / _BGR; a grey stream is replicated), or [height, width, 1] (LOCOV_JPEG_L, grey streams only); contiguous,
 * aligned to one byte only.  EVERY byte of every output is written, nothing else; every workspace byte that is read was written by
 * the call.  Two launches, no host read, no atomics, no memset, integer arithmetic only:
 *   1  all 8x8 blocks of all images: eight lanes own a block (a column each, then a row each; a wave holds eight blocks).  The
 *      wave zero-fills its blocks in LDS, scatters entry * quantiser into them, runs jidctint's column pass (descale 11) and row
 *      pass (descale 18) with the transposition through LDS, and writes range-limited bytes -- the table of jdmaster.c indexed by
 *      x & 1023, level shift included -- into the image's per-component planes in the workspace;
 *   2  16 x 64 output tiles: the planes are read with neighbours clamped at the component's REAL downsampled size
 *      ceil(W * h / hmax) x ceil(H * v / vmax); a chroma plane of half the width is upsampled by jdsample.c's h2v1 / h2v2 "fancy"
 *      filters when that real width exceeds 2 and by replication otherwise; jdcolor.c's 16-bit fixed-point YCbCr -> RGB, a
 *      clamp, and HWC stores through LDS as whole dwords.
 * The bytes are locov_amd.jpeg.decode_jpeg_host's.  A word of a record that lies outside its image (an index past the entries, a
 * coefficient index past 63) cannot make the kernels read or write out of bounds: starts are clamped to the image's entry count and
 * indices masked.
 * n_images == 0: LOCOV_OK, nothing is touched.  More than LOCOV_LABEL_MAX_IMAGES images, a null pointer, a size outside
 * 1 .. 65535, a layout outside the three above, L for a colour image, offsets that are misaligned or leave `records`, a
 * record_bytes smaller than the block starts, a workspace that is misaligned (16) or too small: LOCOV_ERR_INVALID_ARG before any
 * HIP call. */
int locov_jpeg_decode(const void *records, int64_t record_bytes, const locov_jpeg_desc *descs_host, int n_images, int format,
                      void *const *outs_host, void *workspace, int64_t workspace_bytes, locov_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* LOCOV_JPEG_H */

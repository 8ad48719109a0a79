/*
 * frad_hip.h -- C-ABI of the MI355X-native FrAD transform core (libfrad_hip.so).
 *
 * Drop-in boundary for ONE hot path of H4n-uL/FrAD_Python: the per-frame Fourier
 * analysis/synthesis + quantise + bit-depth pack/unpack that the reference reaches only through
 * the two `match` dispatches
 *      src/libfrad/encoder.py:96-100   fourier.profileN.analogue(frame, bits, srate, endian|loss_level)
 *      src/libfrad/decoder.py:70-74    fourier.profileN.digital(frad, depth_idx, channels, ...)
 * Each entry point below replaces one of those Python functions with ONE batched launch over
 * `n_frames` independent frames of identical geometry.  The reference has no FFI of its own
 * (it is pure Python); INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) owned by the caller; nothing is allocated per call
 *    except the immutable twiddle tables, created once per (N, precision) -- call
 *    frad_plan_prepare() first if the launch must be hipGraph-capturable;
 *  - all work is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *  - return value: FRAD_OK (0) or a negative frad_status; never exit(), never throws;
 *  - "sample-frame" = one sample of every channel; PCM is interleaved [n, C] exactly as the
 *    reference reshapes it (encoder.py:84);
 *  - there is NO CPU fallback: without a HIP device every launch returns FRAD_E_HIP.
 */
#ifndef FRAD_HIP_H
#define FRAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRAD_ABI_VERSION 1

typedef enum frad_status {
    FRAD_OK = 0,
    FRAD_E_INVALID = -1,      /* bad argument (null pointer, illegal depth, N or C out of range)   */
    FRAD_E_UNSUPPORTED = -2,  /* legal in the reference but not built here yet (see strerror)      */
    FRAD_E_HIP = -3,          /* a HIP runtime call failed; frad_last_hip_error() has the code     */
    FRAD_E_NOMEM = -4
} frad_status;

/* PCM element type: kind*8 + log2(itemsize)*2 + big_endian, kind 0 = unsigned int, 1 = signed
 * int, 2 = IEEE float.  Replaces ff_format_to_numpy_type (src/libfrad/backend/pcmformat.py:4-32). */
#define FRAD_PCM_CODE(kind, log2size, be) ((kind) * 8 + (log2size) * 2 + (be))
enum {
    FRAD_PCM_U8 = 0, FRAD_PCM_U16LE = 2, FRAD_PCM_U16BE = 3, FRAD_PCM_U32LE = 4, FRAD_PCM_U32BE = 5,
    FRAD_PCM_U64LE = 6, FRAD_PCM_U64BE = 7,
    FRAD_PCM_S8 = 8, FRAD_PCM_S16LE = 10, FRAD_PCM_S16BE = 11, FRAD_PCM_S32LE = 12, FRAD_PCM_S32BE = 13,
    FRAD_PCM_S64LE = 14, FRAD_PCM_S64BE = 15,
    FRAD_PCM_F16LE = 18, FRAD_PCM_F16BE = 19, FRAD_PCM_F32LE = 20, FRAD_PCM_F32BE = 21,
    FRAD_PCM_F64LE = 22, FRAD_PCM_F64BE = 23
};

/* flags */
#define FRAD_LITTLE_ENDIAN 1u /* payload endianness (ASFH `endian`, tools/asfh.py:6-10); 12-bit is always BE */
#define FRAD_RAW_BE_INTS   2u /* reproduce the reference's to_f64 quirk: big-endian integer PCM is NOT
                                 normalised (pcmformat.py:37-45 compares against native dtypes only)  */

/* ---- tables / bookkeeping ------------------------------------------------------------------ */
int         frad_abi_version(void);
const char* frad_strerror(int status);
int         frad_last_hip_error(void);
/* payload bytes of one frame: N*C*bits/8, 12-bit rounds the nibble count up (profile0.py:33-41). */
size_t      frad_payload_bytes(int32_t N, int32_t C, int32_t bits);
/* 1 if frad_p0_* runs the LDS-resident FFT kernel for this N (else the generic direct-sum kernel). */
int         frad_has_fast_path(int32_t N, int32_t C, int32_t compute_f32);
/* build the twiddle tables for (N, precision) on the current device now (hipMalloc + upload).   */
int         frad_plan_prepare(int32_t N, int32_t compute_f32);
void        frad_plan_clear(void);

/* ---- profile 0: DCT archiving ----------------------------------------------------------------
 * frad_p0_analogue  == fourier.profile0.analogue (src/libfrad/fourier/profile0.py:14-44) fused with
 * to_f64 (backend/pcmformat.py:34-47) and the frame cut (encoder.py:72-93), batched.
 *   pcm            first sample-frame of frame 0; frame i starts `frame_stride` sample-frames later
 *   pcm_dtype      FRAD_PCM_*; integer and f64 input is transformed in f64, f32/f16 input in f32
 *                  (the reference does not widen floats and pocketfft then stays in single)
 *   bits           storage depth 12/16/24/32/48/64 (the caller applies `bits not in DEPTHS -> 16`)
 *   payload        frame i's bytes start at payload + i*payload_stride (>= frad_payload_bytes)
 *   absmax[i]      max |X| of frame i as float64 (NaN if any bin is NaN, like np.max): the caller
 *                  compares it with the storage type's max and re-submits the rare frame that
 *                  needs a deeper format (profile0.py:24-26).  May be NULL.
 */
int frad_p0_analogue(const void* pcm, int32_t pcm_dtype, int64_t n_frames, int32_t N, int32_t C,
                     int64_t frame_stride, int32_t bits, uint32_t flags,
                     void* payload, int64_t payload_stride, double* absmax, void* stream);

/* frad_p0_analogue with the reference's per-frame overflow test (profile0.py:24-26) applied in the same pass:
 * *overflow_flag is set to 1 when any frame's max|X| exceeds the storage float's largest finite value (NaN does not
 * count, as in the reference), and left alone otherwise.  The N = 2048 wave kernels test as they go; every other
 * geometry runs frad_p0_overflow_scan behind the transform on the same stream.  `absmax` is required.              */
int frad_p0_analogue_checked(const void* pcm, int32_t pcm_dtype, int64_t n_frames, int32_t N, int32_t C,
                             int64_t frame_stride, int32_t bits, uint32_t flags, void* payload, int64_t payload_stride,
                             double* absmax, int32_t* overflow_flag, void* stream);
/* The overflow test of profile0.py:24-26 over a batch, on the device: *flag |= 1 if any absmax[i] is
 * greater than the largest finite value of the `bits` storage float (NaN never is, like numpy's
 * comparison).  `flag` is a device int32 the caller zeroes once and reads when it needs the answer
 * (sticky across calls), so a steady stream of batches needs no host round trip per batch.        */
int frad_p0_overflow_scan(const double* absmax, int64_t n_frames, int32_t bits, int32_t* flag, void* stream);

/* frad_p0_digital == fourier.profile0.digital (profile0.py:46-69): unpack, NaN/Inf -> 0, inverse
 * DCT in float64, [N, C] interleaved float64 out (frame i at pcm_out + i*N*C).                    */
int frad_p0_digital(const void* payload, int64_t payload_stride, int64_t n_frames, int32_t N, int32_t C,
                    int32_t bits, uint32_t flags, double* pcm_out, void* stream);

/* A batch of equally cut CLIPS consumed and produced in place (BASELINE config 3: 4096 x 1 s clips; the reference cuts
 * every clip into frames on its own, src/libfrad/encoder.py:72-93, and its decoder returns them clip by clip):
 * frad_p0_analogue_clips == frad_p0_analogue_checked over frames (clip c, i), i < frames_per_clip, read at
 * pcm + (c*clip_stride + i*N) sample-frames -- the resident layout [n_clips, clip_stride, C] -- with the payloads dense,
 * frame c*frames_per_clip + i at payload + (c*frames_per_clip + i)*payload_stride (absmax likewise; overflow_flag may be
 * NULL).  A clip's shorter last frame is one more call with frames_per_clip = 1, its own N, and `pcm` advanced to the first
 * clip's tail.  frad_p0_digital_clips == frad_p0_digital writing frame (c, i) at pcm_out + (c*out_clip_stride + i*N)*C.
 * The N = 2048 wave kernels and the any-N Bluestein kernels address clips themselves; every other geometry goes through
 * one strided device copy to / from stream-ordered scratch.  clip_stride >= frames_per_clip*N.                       */
int frad_p0_analogue_clips(const void* pcm, int32_t pcm_dtype, int64_t n_clips, int64_t clip_stride, int32_t frames_per_clip,
                           int32_t N, int32_t C, int32_t bits, uint32_t flags, void* payload, int64_t payload_stride,
                           double* absmax, int32_t* overflow_flag, void* stream);
int frad_p0_digital_clips(const void* payload, int64_t payload_stride, int64_t n_clips, int32_t frames_per_clip, int32_t N,
                          int32_t C, int32_t bits, uint32_t flags, double* pcm_out, int64_t out_clip_stride, void* stream);

/* ---- profile 4: PCM archiving (same pack/unpack, no transform; profile4.py:14-41, 43-63) ------
 * float32/float16 PCM is cast from single precision, everything else from float64, as numpy's
 * astype does on the reference's arrays.                                                          */
int frad_p4_analogue(const void* pcm, int32_t pcm_dtype, int64_t n_frames, int32_t N, int32_t C,
                     int64_t frame_stride, int32_t bits, uint32_t flags,
                     void* payload, int64_t payload_stride, double* absmax, void* stream);
int frad_p4_digital(const void* payload, int64_t payload_stride, int64_t n_frames, int32_t N, int32_t C,
                    int32_t bits, uint32_t flags, double* pcm_out, void* stream);

/* ---- profile 1: psychoacoustic quantiser, pre-/post-entropy halves ----------------------------
 * frad_p1_analogue == fourier.profile1.analogue up to the two integer arrays (profile1.py:15-40 with
 * p1tools.py:15-44).  `N` must be a legal compact frame size (fourier/profiles.py:14-23); frame i
 * reads `n_valid` (<= N) sample-frames starting at pcm + i*frame_stride (frame_stride = hop when the
 * encoder overlaps, encoder.py:35-51) and is zero-padded to N (profile1.py:19).
 *   q   int32 [n_frames, N, C]  bin-major / channel-minor   (freqs_flat, profile1.py:34-36)
 *   tq  int32 [n_frames, 27, C] band-major / channel-minor  (thres_flat, profile1.py:38-40)
 * The Exp-Golomb-Rice stage that follows (profile1.py:43-45) is frad_p1_golomb_encode below; zlib's deflate
 * (profile1.py:50) stays on the host.
 *
 * Parity (integer and f64 PCM): q and tq are the reference's integers exactly -- asserted over the depths 8 .. 64, the table
 * rates, loss levels 0.125 .. 50 and either setting of FRAD_RAW_BE_INTS.  The one deviation: the transform is not pocketfft's
 * (the two agree to 8 eps log2(N) max|X|), so where the reference's own rounding is undecided within that bound -- a value that
 * close to a half-integer -- either neighbour may be written.  f32 / f16 PCM (the reference's float32 path): |dq| <= 1 on at
 * most 2 % of the values.
 * The N = 2048, C <= 2 wave kernel decides in float32 and takes only integer PCM whose type and depth bound the scaled
 * coefficients by peak <= 2^31 (its thresholds use a float32 reciprocal of rms^4) with peak^0.8 x loss inside the 256-entry
 * band-code table; f64 PCM, deeper depths and louder unscaled big-endian integers run through the float64 one-shot kernel. */
int frad_p1_analogue(const void* pcm, int32_t pcm_dtype, int64_t n_frames, int32_t N, int32_t C,
                     int64_t frame_stride, int32_t n_valid, int32_t bits, int32_t srate, double loss_level,
                     uint32_t flags, int32_t* q, int32_t* tq, void* stream);

/* frad_p1_digital == fourier.profile1.digital from the decoded integers on (profile1.py:65-77):
 * dequantise, spread the 27 thresholds over the bins, inverse DCT -> float64 [n_frames, N, C].
 *
 * frad_p1_overlap_add == Decoder.overlap over a batch of decoded frames (decoder.py:28-46 with the Hann ramp of
 * backend/__init__.py:3), for overlap_ratio > 1: cut = N*(ratio-1)/ratio; frame i contributes rows [0, cut) to
 * ola_out [n_frames, cut, C], its first N - cut rows cross-faded against frame i-1's tail (`prev_tail`
 * [N - cut, C] for i = 0, NULL = no previous frame: no fade); the last frame's tail is returned in `next_tail`
 * [N - cut, C] for the next batch (or the flush).  The ramp is a table computed on the host, in float64 with
 * the host's cos, so the cross-faded samples are the reference's bit for bit.                           */
int frad_p1_digital(const int32_t* q, const int32_t* tq, int64_t n_frames, int32_t N, int32_t C,
                    int32_t bits, int32_t srate, double* pcm_out, void* stream);
int frad_p1_overlap_add(const double* frames, int64_t n_frames, int32_t N, int32_t C, int32_t overlap_ratio,
                        const double* prev_tail, double* ola_out, double* next_tail, void* stream);

/* ---- profile 1: Exp-Golomb-Rice stage (row 8f #2) ------------------------------------------------
 * frad_p1_golomb_encode == the two exp_golomb_rice_encode calls and the struct.pack of profile1.py:43-45
 * (tools/p1tools.py:46-60): per frame the pre-deflate body  '>I' len(thres_gol) + thres_gol + freqs_gol  is
 * written at bodies + i*body_stride and its length to body_bytes[i].  body_stride >= frad_p1_golomb_bound(N, C)
 * (the worst case: k is taken from the frame's maximum, so a value costs at most k + 3 <= 35 bits), a multiple
 * of 4; `bodies` 4-byte aligned.  q / tq as frad_p1_analogue writes them.  zlib's deflate stays on the host.
 *
 * frad_rows_compact: offsets[0] = 0, offsets[i+1] = offsets[i] + row_bytes[i] (n_rows + 1 entries), and, when `out`
 * is not NULL, row i's first row_bytes[i] bytes copied to out + offsets[i] -- the batch then goes to the host as ONE
 * copy of exactly the bytes deflate needs.  The gather reads a row as aligned 32-bit words: every row needs
 * row_bytes[i] + 4 <= row_stride (frad_p1_golomb_bound includes that slack); rows that violate it are refused
 * with FRAD_E_INVALID only when row_stride < 4 -- the per-row lengths live on the device.
 *
 * frad_p1_golomb_decode == the two exp_golomb_rice_decode calls of profile1.py:59-64 (p1tools.py:62-74) plus untrim
 * (profile1.py:12-13): frame i's inflated body is bodies[offsets[i] .. offsets[i+1]); q [n_frames, N, C] and
 * tq [n_frames, 27, C] receive the decoded integers, zero-filled where the stream ends early and cut at N*C / 27*C
 * values; values outside int32 (only a corrupt stream has them) saturate.  status[i] (may be NULL) = 1 when the body
 * is shorter than its length word.  `bodies` needs 8 readable bytes after offsets[n_frames] (the streams are read as
 * aligned 32-bit words) and must not be NULL even when every body is empty.
 * Deviation on damaged streams only: missing band codes are zero-filled as INTEGERS (threshold (e/2)^0 = 1), where
 * the reference pads the dequantised thresholds with 0.0 (profile1.py:63-65) and thereby silences the affected bins. */
size_t frad_p1_golomb_bound(int32_t N, int32_t C);
int frad_p1_golomb_encode(const int32_t* q, const int32_t* tq, int64_t n_frames, int32_t N, int32_t C,
                          void* bodies, int64_t body_stride, int64_t* body_bytes, void* stream);
int frad_rows_compact(const void* rows, int64_t row_stride, const int64_t* row_bytes, int64_t n_rows, void* out,
                      int64_t* offsets, void* stream);
int frad_p1_golomb_decode(const void* bodies, const int64_t* offsets, int64_t n_frames, int32_t N, int32_t C,
                          int32_t* q, int32_t* tq, int32_t* status, void* stream);

/* ---- profile 2 (TNS) decode: fourier/profile2.py:58-91, tools/p2tools.py ------------------------------------------------
 * frad_p2_golomb_decode == the three exp_golomb_rice_decode calls + untrim of profile2.digital (profile2.py:64-76): frame
 * i's inflated body bodies[offsets[i] .. offsets[i+1]) is '>H' lpc_len | lpc_gol | '>I' thres_len | thres_gol | freqs_gol.
 * lpc [n_frames, 13, C] receives the LPC integers (cut at 13*C, zero-filled), q / tq what frad_p1_golomb_decode writes
 * for the rest of the body.  Same buffer rules (8 bytes of slack after the last body).
 * Deviation on damaged streams only: a body too short for its '>H' word, or whose lpc_len leaves no room for the '>I'
 * word, makes the reference raise (struct.error); here status[i] = 1 and all three arrays of that frame are zero-filled
 * (a frame of zeros).  The profile-1 deviation above (missing band codes zero-filled as integers) applies as well.
 *
 * frad_p2_synth == profile2.digital's dequantisation (profile2.py:69-86): per frame and channel the coefficients
 * dequant(q) / 2^(bits-1), filtered by tns_synthesis (p2tools.py:105-115: scipy.signal.lfilter([1], [1, lpc[1:]/15]),
 * skipped when all 13 integers are 0, discarded when a result is NaN / Inf or above 1e6 in magnitude), times
 * mapping_from_opus of the thresholds (e/2)^quant(tq) -- written as float64 coeffs_out [n_frames, N, C].  That plane is
 * a 64-bit little-endian profile-0 payload: frad_p0_digital(coeffs_out, N*C*8, n_frames, N, C, 64, FRAD_LITTLE_ENDIAN)
 * finishes profile2.digital with idct(norm='forward').  bits: one of profile2.DEPTHS (8, 10, 12, 14, 16, 20, 24), else
 * FRAD_E_INVALID; N a compact frame size, 1 <= C <= 64.
 * Deviation on damaged streams only: frad_p0_digital turns NaN / +-Inf coefficients into 0 (profile0.py:64), where
 * profile2.digital hands them to the IDCT; only a corrupt threshold code makes them. */
int frad_p2_golomb_decode(const void* bodies, const int64_t* offsets, int64_t n_frames, int32_t N, int32_t C,
                          int32_t* q, int32_t* tq, int32_t* lpc, int32_t* status, void* stream);
int frad_p2_synth(const int32_t* q, const int32_t* tq, const int32_t* lpc, int64_t n_frames, int32_t N, int32_t C, int32_t bits,
                  int32_t srate, double* coeffs_out, void* stream);

/* ---- profile 2 (TNS) encode: fourier/profile2.py:15-55, tools/p2tools.py:55-103 ------------------------------------------
 * frad_p2_analogue == profile2.analogue up to the three integer arrays.  Geometry as frad_p1_analogue (N a compact frame size,
 * frame i reads `n_valid` <= N sample-frames at pcm + i*frame_stride, zero-padded to N), 1 <= C <= 64; bits one of
 * profile2.DEPTHS (8, 10, 12, 14, 16, 20, 24), else FRAD_E_INVALID (the caller applies `bits not in DEPTHS -> 16`).
 *   q    int32 [n_frames, N, C]   bin-major / channel-minor  (freqs_flat, profile2.py:38-40)
 *   tq   int32 [n_frames, 27, C]  band-major / channel-minor (thres_flat, profile2.py:42-44)
 *   lpc  int32 [n_frames, 13, C]  the quantised LPC, lpc[:, 0, :] == 0, all 13 zero where tns_analysis keeps the masked
 *        spectrum (lpc_flat, profile2.py:46)
 * exactly the layout frad_p2_golomb_decode writes, so the three arrays go to frad_p2_synth as they are.  The DCT is profile 0's
 * (frad_p0_analogue at 64-bit little-endian storage, into stream-ordered scratch of n_frames*N*C*8 bytes); the masking, the
 * TNS analysis and the quantiser run in k_p2_analysis, one block per (frame, channel).
 * Parity: the thresholds and the LPC integers are the reference's, the quantised coefficients within |dq| <= 1
 * on a small fraction of values (the transform is not pocketfft's).  Deviations, all in the last bits of quantities that are
 * only compared or rounded: the band energies, the means of lpc_cond / calc_autocorr / predgain and the autocorrelation are
 * block sums, not numpy's pairwise sums or np.correlate's BLAS dot products; a frame whose statistic lands within a few ulps of
 * one of tns_analysis's thresholds (1e-10, 0.5, 0.01, 1e6, MIN_PRED) or an LPC value within an ulp of a rounding boundary can
 * decide differently.  The FIR residual itself is np.convolve's arithmetic bit for bit (a sequential fused multiply-add from
 * the oldest tap, as the reference platform's BLAS dot computes it).
 *
 * frad_p2_golomb_encode == the three exp_golomb_rice_encode calls and the struct.pack of profile2.py:48-52: per frame the
 * pre-deflate body  '>H' len(lpc_gol) | lpc_gol | '>I' len(thres_gol) | thres_gol | freqs_gol  at bodies + i*body_stride, its
 * length in body_bytes[i]; body_stride >= frad_p2_golomb_bound(N, C), a multiple of 4, `bodies` 4-byte aligned.  The rows
 * go to frad_rows_compact as profile 1's do; deflate stays on the host. */
int frad_p2_analogue(const void* pcm, int32_t pcm_dtype, int64_t n_frames, int32_t N, int32_t C, int64_t frame_stride,
                     int32_t n_valid, int32_t bits, int32_t srate, double loss_level, uint32_t flags,
                     int32_t* q, int32_t* tq, int32_t* lpc, void* stream);
size_t frad_p2_golomb_bound(int32_t N, int32_t C);
int frad_p2_golomb_encode(const int32_t* q, const int32_t* tq, const int32_t* lpc, int64_t n_frames, int32_t N, int32_t C,
                          void* bodies, int64_t body_stride, int64_t* body_bytes, void* stream);

/* ---- raw DEFLATE inflate (row 8f #1): zlib.decompress(frad, wbits=-15) of the compact profiles (profile1.py:59,
 * profile2.py:61-64) ------------------------------------------------------------------------------------------------------
 * frad_inflate_raw: frame i is the raw DEFLATE stream (RFC 1951: no zlib / gzip wrapper, no preset dictionary)
 * src[src_offsets[i] .. src_offsets[i+1]); it is inflated into dst + i*dst_stride, at most dst_stride bytes.
 *   status[i]     0 = ok: dst_bytes[i] bytes were written and they equal zlib.decompress(stream, wbits=-15);
 *                 1 = invalid or truncated: zlib rejects the stream (the rules of zlib's inflate, bytes after the final
 *                     block ignored, an empty stream invalid);
 *                 2 = the output would exceed dst_stride bytes.
 *                 With a non-zero status dst_bytes[i] = 0 and the row's contents are unspecified (nothing is written
 *                 outside the row).
 * src_offsets: n_frames + 1 non-decreasing entries (DEVICE int64); the source is read bytewise and never outside
 * [src_offsets[0], src_offsets[n_frames]), so `src` needs neither alignment nor slack.  dst 16-byte aligned, dst_stride a
 * positive multiple of 16 (frad_p1_golomb_bound / frad_p2_golomb_bound are); dst_bytes int64 [n_frames], status int32
 * [n_frames].  Only the bytes [0, dst_bytes[i]) of a row are written.  FRAD_E_INVALID for a NULL pointer or a stride /
 * alignment outside these rules.  One wave per frame; LDS per wave about 6 KiB + min(dst_stride, 32 KiB). */
int frad_inflate_raw(const void* src, const int64_t* src_offsets, int64_t n_frames, void* dst, int64_t dst_stride,
                     int64_t* dst_bytes, int32_t* status, void* stream);

/* ---- raw DEFLATE deflate (row 8f #1): zlib.compress(frad, wbits=-15) of the compact profiles (profile1.py:50,
 * profile2.py:54), i.e. zlib.compressobj(-1, zlib.DEFLATED, -15): compress(body) + flush() ------------------------------------
 * frad_deflate_raw: frame i's body src[src_offsets[i] .. src_offsets[i+1]) is deflated into dst + i*dst_stride.
 *   status[i]     0 = ok: the row's first dst_bytes[i] bytes are exactly zlib's raw deflate of the body at level 6
 *                     (Z_DEFAULT_COMPRESSION: lazy matching, good 8 / lazy 16 / nice 128 / chain 128), memLevel 8, window
 *                     bits 15, Z_DEFAULT_STRATEGY;
 *                 1 = the body is 65 274 bytes or longer (wsize + MAX_DIST, where zlib starts sliding its window): it is
 *                     not deflated here, the caller deflates it on the host;
 *                 2 = the body is longer than dst_stride admits (frad_deflate_stride of its length exceeds dst_stride).
 *                 With a non-zero status dst_bytes[i] = 0 and nothing is written to the row.
 * dst_stride: a multiple of 16, at least frad_deflate_stride(longest body) = round16(n + 6 * (n / 16383 + 1) + 1): zlib's
 * worst case for n bytes, stored blocks included (each of the at most n / 16383 + 1 blocks adds at most 42 bits, the
 * final byte boundary at most 7).  dst 16-byte aligned; dst_bytes int64 [n_frames], status int32 [n_frames].  Only the
 * bytes [0, dst_bytes[i]) of a row are written; the source is read bytewise and never outside
 * [src_offsets[0], src_offsets[n_frames]), so neither buffer needs slack.  FRAD_E_INVALID for a NULL pointer or a stride /
 * alignment outside these rules.  One wave per frame; LDS per wave about 12.5 KiB + 6 B per byte of the longest body the
 * stride admits (the body itself is read from global memory when that would exceed 160 KiB).
 * frad_deflate_stride: the smallest dst_stride for bodies of at most max_body_bytes bytes (lengths of 65 274 and more
 * count as 65 273: such bodies get status 1); FRAD_E_INVALID for a negative length. */
int frad_deflate_raw(const void* src, const int64_t* src_offsets, int64_t n_frames, void* dst, int64_t dst_stride,
                     int64_t* dst_bytes, int32_t* status, void* stream);
int64_t frad_deflate_stride(int64_t max_body_bytes);

/* ---- frame header checksum (row 8f #1) --------------------------------------------------------
 * crc_out[i] = zlib.crc32 of the `nbytes` payload bytes of frame i (at data + i*stride), the value
 * ASFH.write puts into a lossless frame's header (src/libfrad/tools/asfh.py:51-73), so a batch's
 * stream can be assembled without a host pass over the payload.                                   */
int frad_crc32_frames(const void* data, int64_t stride, int64_t n_frames, int64_t nbytes, uint32_t* crc_out, void* stream);

/* ---- Reed-Solomon frame protection (src/libfrad/tools/ecc.py: reedsolo.RSCodec(codesize, dsize + codesize), GF(2^8) over
 * 0x11d, alpha = 2, first consecutive root 0) ------------------------------------------------------------------------------
 * A batch is n_frames byte strings back to back: frame f is in[in_off[f] .. in_off[f+1]) and its output goes to
 * out[out_off[f] .. out_off[f+1]); blk_off[f+1] - blk_off[f] is its block count, blk_off[0] = 0, n_blocks = blk_off[n_frames].
 * in_off / blk_off / out_off are DEVICE int64 arrays of n_frames + 1 entries that the caller fills as below; `in` and `out`
 * must be 16-byte aligned.
 * frad_rs_encode == ecc.encode (ecc.py:6-12) of every frame: blocks of dsize bytes (the last may be shorter), each written
 * as data || codesize check bytes.  blk_off[f+1] - blk_off[f] = ceil(len_f / dsize), out_len_f = len_f + blocks_f * codesize.
 * 1 <= dsize, 0 <= codesize, dsize + codesize <= 255.
 * frad_rs_repair == ecc.decode(..., repair=True) (ecc.py:14-25) of every frame: blocks of dsize + codesize stored bytes, each
 * replaced by its data part (block length - codesize bytes, none when the block is not longer than codesize), corrected
 * when a codeword lies within codesize / 2 byte errors of the block and zero-filled otherwise.  blocks_f =
 * ceil(len_f / (dsize + codesize)), out_len_f = len_f - codesize * blocks_f + (codesize - len of a last block shorter than
 * codesize, if any).  corrected[f] / failed[f] (device int32 [n_frames]) count frame f's blocks that needed a correction
 * and got one / could not be corrected.  `work` is device int32 scratch of n_blocks + 1 entries.
 * 0 <= dsize, 0 <= codesize, 1 <= dsize + codesize <= 255. */
int frad_rs_encode(const void* in, const int64_t* in_off, const int64_t* blk_off, const int64_t* out_off, int64_t n_frames,
                   int64_t n_blocks, int32_t dsize, int32_t codesize, void* out, void* stream);
int frad_rs_repair(const void* in, const int64_t* in_off, const int64_t* blk_off, const int64_t* out_off, int64_t n_frames,
                   int64_t n_blocks, int32_t dsize, int32_t codesize, void* out, int32_t* corrected, int32_t* failed,
                   int32_t* work, void* stream);
/* frad_rs_encode_frames == frad_rs_encode of n_frames payloads of the same length `nbytes` (the lossless profiles' batches),
 * without offset arrays: frame f is read from in + f * in_stride and ecc.encode of it, P = nbytes + ceil(nbytes / dsize) *
 * codesize bytes, is written to out + f * out_stride.  Only those P bytes of each output row are written, so the row may
 * start behind a frame header and the gaps between rows stay untouched.  Same code as frad_rs_encode; in and out are
 * device memory of any alignment and must not overlap; with n_frames > 1, in_stride >= nbytes and out_stride >= P.
 * 1 <= dsize, 0 <= codesize, dsize + codesize <= 255.
 * frad_crc16_ansi_frames: crc_out[f] = common.crc16_ansi (reflected polynomial 0xA001, initial value 0, no final XOR) of
 * data[offsets[f] .. offsets[f+1]), the checksum a compact-profile ECC header stores (tools/asfh.py).  offsets is a DEVICE
 * int64 array of n_frames + 1 non-decreasing entries, crc_out device uint16 [n_frames]; any alignment. */
int frad_rs_encode_frames(const void* in, int64_t in_stride, int64_t n_frames, int64_t nbytes, int32_t dsize, int32_t codesize,
                          void* out, int64_t out_stride, void* stream);
int frad_crc16_ansi_frames(const void* data, const int64_t* offsets, int64_t n_frames, uint16_t* crc_out, void* stream);

/* ---- decoder output conversion (R1 epilogue) and native frame-header scan (row 8f #1) ------------------------------
 * frad_from_f64 == backend.pcmformat.from_f64 followed by .astype(fmt) as the reference's caller applies it to every
 * decoded block (backend/pcmformat.py:49-62, src/decoder.py:23): float64 [n_values] -> `out_dtype` (FRAD_PCM_*), floats
 * rounded to nearest even, integers scaled and truncated; samples outside the integer range come out as numpy's astype
 * leaves them on x86-64 (cvttsd2si: low bits of the 32/64-bit conversion, 0x80..0 on overflow and for NaN).
 * flags: FRAD_RAW_BE_INTS reproduces the reference's quirk that big-endian integer formats are not recognised by
 * from_f64 (pcmformat.py:52-60 compares against native dtypes), so the unscaled float64 samples are truncated;
 * FRAD_LITTLE_ENDIAN is the payload endianness as in frad_p{0,4}_digital.
 * frad_p{0,4,1}_digital_pcm == frad_p{0,4,1}_digital with that conversion applied on the way out (profile 4: fused into
 * the unpack; profile 0 / 1: a second pass over stream-ordered scratch), pcm_out [n_frames, N, C] of out_dtype.    */
int frad_from_f64(const double* pcm, int64_t n_values, int32_t out_dtype, uint32_t flags, void* out, void* stream);
int frad_p0_digital_pcm(const void* payload, int64_t payload_stride, int64_t n_frames, int32_t N, int32_t C, int32_t bits,
                        uint32_t flags, int32_t out_dtype, void* pcm_out, void* stream);
int frad_p4_digital_pcm(const void* payload, int64_t payload_stride, int64_t n_frames, int32_t N, int32_t C, int32_t bits,
                        uint32_t flags, int32_t out_dtype, void* pcm_out, void* stream);
/* frad_p1_overlap_add_pcm == frad_p1_overlap_add with that conversion applied on the way out: ola_out [n_frames, cut, C] of
 * out_dtype in one pass over the decoded frames (next_tail stays float64: it is the next batch's input).            */
int frad_p1_overlap_add_pcm(const double* frames, int64_t n_frames, int32_t N, int32_t C, int32_t overlap_ratio, const double* prev_tail,
                            int32_t out_dtype, uint32_t flags, void* ola_out, double* next_tail, void* stream);
int frad_p1_digital_pcm(const int32_t* q, const int32_t* tq, int64_t n_frames, int32_t N, int32_t C, int32_t bits,
                        int32_t srate, int32_t out_dtype, uint32_t flags, void* pcm_out, void* stream);
/* frad_clips_overlap_add == Decoder.overlap + flush() (decoder.py:28-46, 110-114) for n_clips independent streams in one pass,
 * with ragged output and the output conversion of frad_p1_overlap_add_pcm (all arrays in device memory).
 *   frames      float64 [clip_frame0[n_clips], N, C]: the equal-length frames, clip after clip; clip j owns frames
 *               [clip_frame0[j], clip_frame0[j+1]) (m_j of them, m_j >= 0)
 *   tails       float64: clip j's last frame of another length is tail_rows[j] rows of C at ELEMENT offset tail_off[j];
 *               tail_rows[j] == 0: the clip has none
 *   out         out_dtype (FRAD_PCM_*, flags as frad_p1_overlap_add_pcm): clip j's samples start at sample-frame out_off[j], and
 *               out_off[j+1] - out_off[j] == m_j * cut + (tail_rows[j] ? tail_rows[j] : (m_j ? N - cut : 0)); out_off has
 *               n_clips + 1 entries, out_rows == out_off[n_clips] (the host's copy: it sizes the launch, and nothing beyond
 *               min(out_rows, out_off[n_clips]) sample-frames is written); sample-frames before out_off[0] are left alone
 *   overlap_ratio 0: cut = N, no fade (lossless profiles and ratio 0: a ragged gather + conversion)
 *   overlap_ratio 2..256: cut = N*(ratio-1)/ratio, L = N - cut.  Inside a clip, frame i > 0 is cross-faded over its first L
 *               rows against rows [cut, N) of frame i-1 with hanning_in_overlap(L) (backend/__init__.py:3), the values of
 *               frad_p1_overlap_add; a clip's first frame is not faded; the last frame of another length is faded over its first
 *               L rows against the last equal-length frame (not when m_j == 0) and written whole; without one, rows [cut, N) of
 *               the last frame follow unfaded (the flush fragment).  Requires tail_rows[j] == 0 or >= L.
 *   tail_win    optional float64 [L]: hanning_in_overlap(L) as the caller computed it.  When given, it weights the last frames
 *               whose own overlap length tail_rows - tail_rows*(ratio-1)/ratio differs from L: the Decoder cross-fades those
 *               on the host, because the carried fragment has another geometry (decoder.py:207-209), and this keeps the result
 *               bit-identical to it.  NULL: every weight is the library's own table of hanning_in_overlap(L), computed on the
 *               host in float64 as numpy does (the device's cos differs from the host's in the last bit now and then).
 * The offsets are the caller's to check (core.clips_overlap_add does); FRAD_E_INVALID for N, C, the ratio and the dtype.      */
int frad_clips_overlap_add(const double* frames, const int64_t* clip_frame0, int64_t n_clips, int32_t N, int32_t C, int32_t overlap_ratio,
                           const double* tails, const int64_t* tail_off, const int32_t* tail_rows, const double* tail_win,
                           int32_t out_dtype, uint32_t flags, void* out, const int64_t* out_off, int64_t out_rows, void* stream);

/* frad_clips_window_add == frad_clips_overlap_add's arithmetic on an arbitrary row range of each clip: sample windows of many
 * streams in one pass, ragged or scattered into a zero-padded batch (all arrays in device memory).  frames, N, C, overlap_ratio,
 * tails, tail_off, tail_rows, tail_win, out_dtype, flags and stream are frad_clips_overlap_add's.
 *   clip_f0     int64 [n_clips], clip_m int32 [n_clips]: clip j's equal-length frames are frames[clip_f0[j] .. clip_f0[j] + clip_m[j])
 *               (clip_m[j] >= 0).  The ranges of different clips may overlap or coincide, and so may their tail_off: the windows of
 *               one stream share the frames decoded for it.
 *   skip        int64 [n_clips]: the first row of clip j's own timeline to produce.  The timeline is the one
 *               frad_clips_overlap_add writes for a clip of those frames and that tail: row r < m * cut is row r % cut of frame
 *               r / cut, faded against row cut + r % cut of the frame before when r % cut < L and r / cut > 0; after m * cut rows
 *               come the tail_rows[j] rows of the tail (its first L rows faded against frame m - 1 when m > 0), or without a tail
 *               the L rows of the flush fragment (m > 0).  Row for row the values are frad_clips_overlap_add's, bit for bit.
 *   valid       int32 [n_clips]: the rows produced, 0 <= valid[j] <= out_off[j+1] - out_off[j], and skip[j] + valid[j] must not
 *               pass the end of the timeline.  The other rows of the clip's span are written as the conversion of 0.0 to out_dtype
 *               (silence in the output format: 0x80 for FRAD_PCM_U8, not the zero byte).
 *   out_off     int64 [n_clips + 1], non-decreasing: it partitions the launch, clip j's span is out_off[j+1] - out_off[j]
 *               sample-frames long.  out_rows == out_off[n_clips] (the host's copy: it sizes the launch; spans beyond
 *               min(out_rows, out_off[n_clips]) are not written).
 *   dst_row     int64 [n_clips] or NULL.  NULL: clip j's span starts at sample-frame out_off[j] of out, as in
 *               frad_clips_overlap_add (sample-frames before out_off[0] are left alone).  Given: the span starts at sample-frame
 *               dst_row[j] of out and out_off only partitions the launch -- one launch per geometry group scatters into a batch
 *               whose rows belong to several groups.  The spans must be disjoint; nothing outside them is written.
 * A span leaves in 16-byte stores where its address allows it (dst_row[j] * C * itemsize a multiple of 16 from an aligned out),
 * element by element elsewhere.  No scratch memory.
 * The tables are the caller's to check (core.clips_window_add does).  FRAD_E_INVALID for N, C, the ratio, the dtype, negative
 * counts and, with rows to write, a null table (dst_row, tail_win, and frames / tails that no clip reads may be NULL); FRAD_OK
 * without a launch for n_clips == 0 or out_rows == 0.                                                                        */
int frad_clips_window_add(const double* frames, const int64_t* clip_f0, const int32_t* clip_m, int64_t n_clips, int32_t N, int32_t C,
                          int32_t overlap_ratio, const double* tails, const int64_t* tail_off, const int32_t* tail_rows, const double* tail_win,
                          const int64_t* skip, const int32_t* valid, const int64_t* dst_row, int32_t out_dtype, uint32_t flags, void* out,
                          const int64_t* out_off, int64_t out_rows, void* stream);

/* frad_clips_carry_add == frad_p1_overlap_add_pcm for n_clips live streams in one pass: every clip is the next run of whole
 * frames of a stream that is still arriving, so it starts from the fragment the stream carried in and ends in the fragment it
 * carries out, not in a flush (all arrays in device memory).  frames, clip_frame0, N, C, overlap_ratio, out_dtype, flags, out,
 * out_off, out_rows and stream are frad_clips_overlap_add's, with the same legal values; cut = N for ratio 0, else
 * N*(ratio-1)/ratio (at least 1), L = N - cut.
 *   out_off     clip j's span is out_off[j+1] - out_off[j] == m_j * cut sample-frames: there is no last frame of another length
 *               and no flush fragment.  Output row f * cut + n of clip j is row n of its frame f.
 *   prev_ptr    NULL, or n_clips pointers: prev_ptr[j] is NULL or the fragment clip j starts from, float64 [L, C], 8-byte
 *               aligned.  A row is faded when L > 0, n < L and either f > 0 or the clip has a fragment: against row cut + n of
 *               frame f - 1, or row n of the fragment, as x = x * w[n]; x = x + p * w[L-1-n] (a rounded multiply, then a rounded
 *               add) with the library's host-computed table w = hanning_in_overlap(L).  These are frad_p1_overlap_add_pcm's bits
 *               for the same frames and prev_tail; a clip without a fragment is not faded in its first frame.
 *   next_ptr    NULL, or n_clips pointers: when m_j > 0, L > 0 and next_ptr[j] is not NULL, rows [cut, N) of clip j's last frame
 *               are copied there, bits unchanged: float64 [L, C] whatever out_dtype is.  A clip with m_j == 0 writes nothing
 *               anywhere, so its pending fragment stays pending.  next_ptr[j] must not alias frames or any prev_ptr[i]: the
 *               caller double-buffers.  With ratio 0 both tables are ignored.
 * Nothing outside the spans and the named fragments is written, nothing beyond min(out_rows, out_off[n_clips]) sample-frames,
 * and sample-frames before out_off[0] are left alone.  No LDS, no scratch memory.
 * The tables are the caller's to check (core.clips_carry_add does).  FRAD_E_INVALID for N, C, the ratio, the dtype, negative
 * counts and, with rows to write, a null frames, clip_frame0, out_off or out; FRAD_OK without a launch for n_clips == 0 (whatever
 * the other arguments are) and for out_rows == 0 (every clip is empty then).                                                 */
int frad_clips_carry_add(const double* frames, const int64_t* clip_frame0, int64_t n_clips, int32_t N, int32_t C, int32_t overlap_ratio,
                         const double* const* prev_ptr, double* const* next_ptr, int32_t out_dtype, uint32_t flags, void* out,
                         const int64_t* out_off, int64_t out_rows, void* stream);

/* frad_clips_resample: polyphase sample-rate conversion of many ragged float64 spans in one pass, with frad_clips_window_add's
 * output side (all arrays in device memory).  The arithmetic is scipy.signal.resample_poly's with default arguments (zero
 * extension, Kaiser beta = 5): with M = max(up, down) and half_len = 10 * M the caller computes, in float64,
 *   taps[k] = sinc((k - half_len) / M) / M * kaiser(2 * half_len + 1, 5.0)[k], normalised to sum 1, times up,   k = 0 .. 2 * half_len
 * and output row n of a stream is
 *   y[n][c] = sum over i ascending of x[i][c] * taps[n * down - i * up + half_len],
 *             max(0, ceil((n * down - half_len) / up)) <= i <= floor((n * down + half_len) / up), i inside the clip's span,
 * evaluated as acc = fma(x, tap, acc) from acc = 0.0 in that order on every path, so a row's bits do not depend on the window
 * that asked for it.  n * down and i * up are 64-bit.
 *   src         float64: clip j's source rows are src_rows[j] rows of C doubles at element offset src_off[j]; they are rows
 *               src_row0[j] .. of the stream's own timeline (src_row0[j] >= 0).  Rows outside the span count as zero: the
 *               stream's ends, or rows the caller knows no output row of the clip reads.  Spans of different clips may overlap
 *               or coincide.  src may be NULL when every src_rows[j] is 0.
 *   out_row0    int64 [n_clips] >= 0: row r < valid[j] of clip j's span is y[out_row0[j] + r].
 *   valid, dst_row, out_off, out_rows, out_dtype, flags, out, stream: frad_clips_window_add's -- rows from valid[j] to the end
 *               of the span are the conversion of 0.0, spans are disjoint, nothing outside them is written, a span leaves in
 *               16-byte stores where its address allows it and element by element elsewhere.
 * A block stages the source rows its run of output rows reads in LDS when the run lies inside one clip and they fit, and reads
 * them from global memory otherwise; the taps are read through L2.  No scratch memory.
 * The tables are the caller's to check (core.clips_resample does).  FRAD_E_INVALID for C < 1, up < 1, down < 1, half_len != 10 *
 * max(up, down), the dtype, negative counts and, with rows to write, a null table (dst_row and src may be NULL); FRAD_OK
 * without a launch for n_clips == 0 or out_rows == 0.                                                                       */
int frad_clips_resample(const double* src, const int64_t* src_off, const int64_t* src_row0, const int32_t* src_rows, int64_t n_clips,
                        int32_t C, int32_t up, int32_t down, const double* taps, int32_t half_len, const int64_t* out_row0,
                        const int32_t* valid, const int64_t* dst_row, int32_t out_dtype, uint32_t flags, void* out, const int64_t* out_off,
                        int64_t out_rows, void* stream);

/* frad_clips_remix: a channel mix of many ragged float64 spans whose channel count differs per clip, in one pass, with
 * frad_clips_window_add's output side (all arrays in device memory).  Clip j has src_ch[j] = C_in channels and a float64 matrix
 * M[C_out][C_in]; for one source row x[0 .. C_in) and output channel k
 *   the terms are the c, ascending, with M[k][c] != 0.0; the first sets acc = x[c] * M[k][c], every later one does
 *   acc = acc + x[c] * M[k][c] -- a rounded multiply, then a rounded add, never an fma; a row of M without a non-zero entry
 *   gives +0.0.
 * Skipping the zero weights is part of the definition: an identity or permutation row copies the source's bits (-0.0,
 * denormals, +-Inf; x * 1.0 is exact), no Inf * 0 is ever formed, and the result equals the elementwise numpy model
 * (window.clips_remix_host) bit for bit for every matrix.
 *   src_ptr     [n_clips] device addresses: clip j's valid[j] rows of src_ch[j] doubles, 8-byte aligned.  A table of pointers,
 *               not a base and offsets: the windows of one call come out of several launches' allocations.  src_ptr[j] may be
 *               NULL where valid[j] == 0.
 *   src_ch      int32 [n_clips] >= 1.
 *   mats        float64; clip j's matrix is the C_out * src_ch[j] doubles at element mat_off[j] (int64 [n_clips]), row-major
 *               [C_out][C_in].  Clips may share one.
 *   valid, dst_row, out_off, out_rows, out_dtype, flags, out, stream: frad_clips_window_add's -- rows from valid[j] to the end
 *               of the span are the conversion of 0.0, spans are disjoint, nothing outside them is written, a span leaves in
 *               16-byte stores where its address allows it and element by element elsewhere.  The launch is partitioned by
 *               out_off in units of C_out elements.
 * A source row's values are read once per row and store, two at a time where the address is 16-byte aligned; the matrices are
 * read through the caches.  No LDS, no scratch memory.
 * The tables are the caller's to check (core.clips_remix does).  FRAD_E_INVALID for C_out < 1, the dtype, negative counts and,
 * with rows to write, a null table (dst_row may be NULL); FRAD_OK without a launch for n_clips == 0 or out_rows == 0.       */
int frad_clips_remix(const double* const* src_ptr, const int32_t* src_ch, const double* mats, const int64_t* mat_off, int64_t n_clips,
                     int32_t C_out, const int32_t* valid, const int64_t* dst_row, int32_t out_dtype, uint32_t flags, void* out,
                     const int64_t* out_off, int64_t out_rows, void* stream);

/* frad_clips_spectrum: power / magnitude / (log-)filterbank spectrogram of many ragged float64 windows in one pass (all arrays
 * in device memory).  Clip j is valid[j] rows of K doubles at src_ptr[j]; every row outside [0, valid[j])
 * counts as +0.0.  With N = n_fft, frame f of a clip and channel c:
 *   x[n]  = row f * hop + n - (center ? N/2 : 0), channel c, times window[n]          n = 0 .. N-1 (a rounded product)
 *   X[k]  = sum_n x[n] exp(-2 pi i k n / N)                                            k = 0 .. N/2, unnormalised, float64
 *   P[k]  = Re^2 + Im^2 (power = 2), or its square root (power = 1)
 *   v[m]  = P[m] (n_bands = 0: N/2 + 1 values), or acc from +0.0 of acc = acc + band_w[band_off[m] + i] * P[band_lo[m] + i],
 *           i = 0 .. band_len[m] - 1 ascending (a rounded multiply, a rounded add; a band of length 0 gives +0.0)
 *   y[m]  = v[m] (log_scale = 0), or v[m] <= floor ? floor_log : log_scale * log(v[m]); floor_log is the caller's
 *           log_scale * log(floor), stored as given, so that every clamped value is one constant whatever the device's log
 *   out   = y rounded to nearest: float32 (out_dtype FRAD_PCM_F32LE) or float64 (FRAD_PCM_F64LE)
 * X is computed as an N/2-point complex FFT of the packed sequence (fft_team, twiddles from the plan tables) and one split
 * pass: the error against the exact sum is that of a radix FFT in float64.  An all-zero frame gives P = +0.0 exactly.  A
 * frame's values depend only on its N inputs and the tables, not on the launch around it.
 *   frame_off   int64 [n_clips + 1], ascending: clip j owns the frames frame_off[j] .. frame_off[j+1] - 1 of the launch, the
 *               first of them its frame 0.  Frames at or beyond out_frames are not computed.
 *   out         [out_frames, K, n_out] values, n_out = n_bands or N/2 + 1: one frame-channel's values are contiguous.  A dense
 *               batch [B, F, K, n_out] is frame_off[j] = j * F.  Nothing else is written.
 *   window      float64 [N]; band_lo, band_len int32 [n_bands]; band_off int64 [n_bands]; band_w float64 [n_weights].
 * N is a power of two from 128 to 4096.  One LDS-resident transform per frame-channel, no scratch memory.
 * The tables are the caller's to check (core.clips_spectrum does); a band that leaves [0, N/2] or band_w is cut short, never
 * read.  FRAD_E_INVALID for N, hop < 1, K < 1, center not 0/1, power not 1/2, the dtype, negative counts, a logarithm without
 * finite floor > 0 and floor_log, and, with frames to write, a null table; FRAD_OK without a launch for n_clips == 0 or
 * out_frames == 0.                                                                                                          */
int frad_clips_spectrum(const double* const* src_ptr, const int32_t* valid, int64_t n_clips, int32_t K, const int64_t* frame_off,
                        int64_t out_frames, int32_t n_fft, int32_t hop, int32_t center, const double* window, int32_t power,
                        int32_t n_bands, const int32_t* band_lo, const int32_t* band_len, const int64_t* band_off, const double* band_w,
                        int64_t n_weights, double log_scale, double floor, double floor_log, int32_t out_dtype, void* out, void* stream);

/* frad_clips_frame_cut == the Encoder's frame cut (encoder.py:72-93) for the frames of many clips in one pass: fixed-length
 * rows gathered from arbitrary sample-frame offsets of ONE buffer that holds all clips back to back (all arrays in device
 * memory).  With rb = row_len * step bytes per row,
 *   out[r * rb, (r + 1) * rb) = src[row_src[r] * step, (row_src[r] + row_valid[r]) * step), then zero bytes up to rb
 *   src         raw interleaved PCM, any alignment; step = itemsize * channels bytes per sample-frame (1 = u8 mono, upwards)
 *   row_src     int64 [n_rows]: the row's first sample-frame in src; rows may overlap (the hop of an overlapped encode)
 *   row_valid   int32 [n_rows]: 0 .. row_len sample-frames taken from src (0: the row is all padding, row_src is not read from)
 *   out         [n_rows, row_len] sample-frames, contiguous, any alignment: the block frad_p{0,1,2,4}_analogue read with
 *               frame_stride = row_len.  Nothing outside its n_rows * rb bytes is written.
 * One read and one write of the PCM, no scratch; the transform kernels' addressing stays as it is.
 * The offsets are the caller's to check (core.clips_frame_cut does): every row_src[r] + row_valid[r] must end inside src.
 * FRAD_E_INVALID for step < 1, row_len < 1, n_rows < 0 and, with rows to write, a null pointer.                          */
int frad_clips_frame_cut(const void* src, const int64_t* row_src, const int32_t* row_valid, int64_t n_rows, int32_t row_len, int32_t step,
                         void* out, void* stream);

/* frad_clips_carry_cut == frad_clips_frame_cut for clips that are pieces of live streams (all arrays in device memory).  Clip j's
 * virtual sequence V_j is carry_len[j] sample-frames at carry_ptr[j], then the sample-frames src[src_off[j] .. src_off[j+1]) of one
 * joined buffer; have_j is their sum.  step = itemsize * channels bytes per sample-frame (1 = u8 mono, upwards, no power of two
 * needed), rb = row_len * step bytes per row.
 *   out         [n_rows, row_len] sample-frames, contiguous, any alignment: row r is V_c[row_at[r] .. row_at[r] + row_len) with
 *               c = row_clip[r] (int32 [n_rows]; row_at int64 [n_rows]).  Every row is whole -- there is no padding -- and may lie in
 *               the carry, in the chunk or across the seam; rows of one clip overlap when the hop is smaller than row_len.  The
 *               block frad_p{0,1,2,4}_analogue read with frame_stride = row_len.
 *   next_ptr    NULL, or n_clips pointers: where next_ptr[j] is not NULL the bytes of V_j[next_at[j] .. have_j) are copied there,
 *               bits unchanged (next_at int64 [n_clips]; it may be zero sample-frames, and it may begin inside the carry: a clip
 *               without a row carries out carry ++ chunk).  next_ptr[j] must not alias out, src or any carry_ptr[i]: the caller
 *               double-buffers.  A clip with a NULL next_ptr[j] writes nothing there.
 *   carry_ptr   n_clips pointers; carry_ptr[j] may be NULL where carry_len[j] == 0 (int32 [n_clips] >= 0).  Carries, src and the
 *               destinations may sit at any byte alignment.
 *   src         never NULL (any address will do when every span is empty); src_off int64 [n_clips + 1], non-decreasing.
 * One launch writes the rows and the remainders.  Nothing outside out's n_rows * rb bytes and the named remainders is written.
 * No LDS, no scratch memory.
 * The tables are the caller's to check (core.clips_carry_cut does): every row must end inside its clip's have_j, 0 <= next_at[j]
 * <= have_j, and src_off must stay inside src.  FRAD_E_INVALID for step < 1, row_len < 1, negative counts, and a null table or
 * buffer with something to read or write through it; FRAD_OK without a launch for n_clips == 0, and for no row and no next_ptr. */
int frad_clips_carry_cut(const void* const* carry_ptr, const int32_t* carry_len, const void* src, const int64_t* src_off,
                         int64_t n_clips, const int32_t* row_clip, const int64_t* row_at, int64_t n_rows, int32_t row_len,
                         int32_t step, void* out, const int64_t* next_at, void* const* next_ptr, void* stream);

/* frad_asfh_scan: HOST code (no device involved).  One pass over a FrAD byte stream from `start`: resynchronises on
 * FRM_SIGN and parses every header as ASFH.read does (tools/asfh.py:98-134; the search as decoder.py:82-90), filling
 * frames[0 .. return value).  Stops at the first header or payload that is not completely inside the buffer, at
 * max_frames, or at the end; *next_pos = where the next call (with more data appended) must resume, *stop_reason says
 * why.  Force-flush headers are table rows with force_flush = 1 and no payload.  A compact header whose sample-rate
 * index is not in the table (>= 12; the reference raises) is reported with srate = 0.  Returns the row count or
 * FRAD_E_INVALID. */
typedef struct frad_frame_info {
    int64_t header_off, payload_off, payload_bytes;
    int32_t profile, ecc, little_endian, depth_idx, channels, srate, fsize, overlap_ratio, ecc_dsize, ecc_codesize, force_flush;
    uint32_t crc;                                 /* crc32 of the payload (lossless) / crc16 (compact with ECC) as stored */
} frad_frame_info;
enum { FRAD_SCAN_END = 0, FRAD_SCAN_PARTIAL_HEADER = 1, FRAD_SCAN_PARTIAL_PAYLOAD = 2, FRAD_SCAN_TABLE_FULL = 3 };
int64_t frad_asfh_scan(const void* stream_bytes, int64_t nbytes, int64_t start, frad_frame_info* frames, int64_t max_frames,
                       int64_t* next_pos, int32_t* stop_reason);

/* ---- measurement aid (not on the codec path) ----------------------------------------------------
 * dst[0, nbytes) = src[0, nbytes): device-to-device, 16 bytes per lane, the access shape of the
 * transform kernels.  bench.py times it as the "achievable HBM bandwidth" yardstick next to the
 * codec kernels.  nbytes and both pointers must be multiples of 16.                                 */
int frad_bench_copy(const void* src, void* dst, int64_t nbytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRAD_HIP_H */

/*
 * spectro_hip.h — C ABI of libspectro_hip.so, the MI355X (gfx950) engine for the
 * batched STFT / Mel-spectrogram hot path of the `spectrograms` crate
 * (jmg049/Spectrograms v2.1.0).  All reference citations are file:line under the
 * reference repository root.
 *
 * This header is the drop-in boundary: a `fft_backend::hip_backend` variant in
 * the reference (the analogue of its FFTW variant, src/fft_backend.rs:1084-1871)
 * binds exactly these symbols — see INTEGRATION.md for the Rust `extern "C"`
 * block and the ctypes binding used by the Python host mirror.
 *
 * Conventions
 *  - Plain C types only; no C++/torch types cross the boundary.
 *  - A plan is the analogue of the reference's `&mut self` plans
 *    (src/fft_backend.rs:21-24: "own scratch, reusable, no heap allocation in
 *    process"): it owns every device table (window, twiddles, filterbank) and all
 *    scratch; it is NOT thread-safe (one caller at a time, like `&mut self`;
 *    Python plan objects are `unsendable`, src/python/planner.rs:674).  Distinct
 *    plans are independent.
 *  - No function aborts or throws across the ABI.  Status codes mirror
 *    `SpectrogramError` (src/error.rs:13-28); the message text is available
 *    from sgx_last_error() / sgx_last_create_error().
 *  - There is no CPU fallback: without a usable HIP device every compute entry
 *    point returns SGX_BACKEND.
 *  - The library keeps no mutable global state and reads no environment
 *    variables; an entry point leaves the caller's current HIP device as it
 *    found it.
 *  - Allocation: everything the per-frame entry points (sgx_r2c / sgx_c2r, the
 *    analogues of R2cPlan / C2rPlan::process) touch is allocated by
 *    sgx_plan_create.  The batched entry points need scratch that depends on the
 *    call's size (host staging, the MFCC Mel tensor, the generic inverse path's
 *    frames): sgx_reserve sizes it ahead; a call that fits what was reserved
 *    allocates nothing, a larger one grows the scratch once.
 *  - Streams (the batched 1-D entry points: sgx_execute, sgx_istft, sgx_mdct_forward / _inverse, sgx_binaural_execute /
 *    _histogram, sgx_gammatone_execute, sgx_fir_process / _convolve / _reset, sgx_deconv_execute, sgx_minphase_execute, sgx_stream_push / _flush, sgx_istream_push / _flush, sgx_resample_resample / _process / _flush / _reset, sgx_welch_execute, sgx_kaldi_execute): a device-pointer call enqueues ALL of its work on `hip_stream` — every launch of a
 *    multi-launch route, the memsets in front of the inverse kernels, every chunk of a long batch — and on nothing else, and
 *    returns without waiting for it: to the caller it is one operation of that stream, ordered behind what was queued there
 *    before and in front of what is queued there afterwards.  A plan's scratch belongs to one in-flight call at a time: calls
 *    on one plan that go to different streams must be ordered by the caller (events), as must a host-pointer call behind a
 *    device-pointer call still in flight.  A call does not depend on the calls before it: a larger, smaller, failed, host- or
 *    device-pointer call in between changes neither the bits nor the route of the next one (the DC / Nyquist flag word is
 *    cleared per call; the one exception is the state a streaming plan exists to carry: sgx_fir_process reads and replaces
 *    the plan's history, sgx_stream_push the stream's pending samples, sgx_istream_push the stream's overlap tail, sgx_resample_process the rows' last K - 1 samples, in stream order).  A device-pointer call that fits what was reserved (host_staging = 0 suffices) allocates nothing, does
 *    not synchronise and copies nothing from the host, so it can be captured into a hipGraph, as a linear chain, and replayed;
 *    a call that has to grow scratch frees and allocates, which waits for the device and cannot be captured.  Pinned per route
 *    by tests/test_stream_order.py, the state-carrying calls as fixed schedules (push, push, flush; reset, process, process, flush)
 *    on one plan; the sgx_fir calls and sgx_deconv_execute by tests/test_fir.py, sgx_minphase_execute by tests/test_minphase.py.
 */
#ifndef SPECTRO_HIP_H
#define SPECTRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGX_ABI_VERSION 7

typedef struct sgx_plan sgx_plan; /* opaque */

/* src/error.rs:13-28  InvalidInput / DimensionMismatch / FftBackendError{backend:"hip"} / InternalError */
typedef enum {
    SGX_OK = 0,
    SGX_INVALID_INPUT = 1,
    SGX_DIM_MISMATCH = 2,
    SGX_BACKEND = 3,
    SGX_INTERNAL = 4
} sgx_status;

/* src/window.rs:19-50 WindowType */
enum { SGX_WIN_RECTANGULAR = 0, SGX_WIN_HANNING = 1, SGX_WIN_HAMMING = 2, SGX_WIN_BLACKMAN = 3,
       SGX_WIN_KAISER = 4, SGX_WIN_GAUSSIAN = 5, SGX_WIN_CUSTOM = 6 };
/* src/spectrogram.rs:3374-3442 frequency-scale markers (LinearHz, Mel, LogHz, Erb).  LogHz (LogHzParams :3935-3990,
 * matrix build_loghz_matrix :2438-2508) reuses n_mels / f_min / f_max as n_bins / f_min / f_max.  Erb (ErbParams
 * src/erb.rs:27-92, frequency-domain gammatone bank ErbFilterbank::generate :266-335, applied as a DENSE
 * n_filters x (n_fft/2+1) product with the power spectrum :374-401) reuses them as n_filters / f_min / f_max. */
enum { SGX_FREQ_LINEAR = 0, SGX_FREQ_MEL = 1, SGX_FREQ_LOGHZ = 2, SGX_FREQ_ERB = 3, SGX_FREQ_CHROMA = 4, SGX_FREQ_CQT = 5 };
/* Chroma (src/chroma.rs): chromagram() :470-505 = linear MAGNITUDE spectrogram -> dense 12 x (n_fft/2+1) pitch-class bank
 * (build_chroma_filterbank :262-345, bins inside [f_min, f_max], Gaussian over the circular semitone distance, rows
 * normalised to unit sum) applied with sequential accumulation (:378-392) -> per-frame normalisation over the 12 rows
 * (apply_chroma_normalization :403-445).  Requires amp_scale = SGX_AMP_MAGNITUDE and no LogParams; f_min / f_max reused;
 * output has 12 rows.  ChromaNorm :24-31: */
enum { SGX_CHROMA_NORM_NONE = 0, SGX_CHROMA_NORM_L1 = 1, SGX_CHROMA_NORM_L2 = 2, SGX_CHROMA_NORM_MAX = 3 };
/* ErbSpacing src/erb.rs:14-25 */
enum { SGX_ERB_LINEAR = 0, SGX_ERB_APPLE_TR35 = 1 };
/* MelNorm src/spectrogram.rs:2385-2429 */
enum { SGX_MELNORM_NONE = 0, SGX_MELNORM_SLANEY = 1, SGX_MELNORM_L1 = 2, SGX_MELNORM_L2 = 3 };
/* AmpScaleSpec impls src/spectrogram.rs:1986-2037; COMPLEX = StftPlan::compute (:1424-1458) */
enum { SGX_AMP_POWER = 0, SGX_AMP_MAGNITUDE = 1, SGX_AMP_DECIBELS = 2, SGX_AMP_COMPLEX = 3 };
/* Sample impls src/sample.rs:23-86 */
enum { SGX_F32 = 0, SGX_F64 = 1 };
enum { SGX_MEM_HOST = 0, SGX_MEM_DEVICE = 1 };

/* StftParams (src/spectrogram.rs:3452-3506) + SpectrogramParams (:4108-4140) + MelParams (:3744-3813)
 * + LogParams (:4052-4077) + the `T: Sample` choice, flattened. */
typedef struct {
    uint32_t n_fft;
    uint32_t hop_size;
    int32_t centre;               /* zero padding of n_fft/2 on both sides (S1) */
    int32_t window_kind;          /* SGX_WIN_* */
    double window_param;          /* Kaiser beta / Gaussian std in samples */
    const double *custom_window;  /* n_fft coefficients (copied) or NULL */
    uint32_t custom_window_len;   /* must equal n_fft for SGX_WIN_CUSTOM (:3490-3498) */
    double sample_rate_hz;
    int32_t freq_scale;           /* SGX_FREQ_* */
    uint32_t n_mels;
    double f_min, f_max;
    int32_t mel_norm;             /* SGX_MELNORM_* */
    int32_t amp_scale;            /* SGX_AMP_* */
    int32_t has_log_params;       /* Option<&LogParams>: dB applied only when set (S6) */
    double floor_db;
    int32_t dtype;                /* SGX_F32 / SGX_F64 */
    int32_t device;               /* HIP device ordinal; -1 = current device; -2 = host-only plan (no compute) */
    /* MfccParams (src/mfcc.rs:20-90): n_mfcc > 0 turns the plan into mfcc_from_log_mel (:224-273) applied to its
     * Mel-dB output — unnormalised DCT-II with an FMA chain in T (:278-292), sinusoidal lifter (:297-316), optional
     * removal of C0.  Requires freq_scale = MEL and amp_scale = DECIBELS; n_mfcc <= n_mels. */
    uint32_t n_mfcc;
    int32_t mfcc_include_c0;
    uint32_t mfcc_lifter;
    int32_t erb_spacing;          /* SGX_ERB_* (only read when freq_scale = SGX_FREQ_ERB) */
    double chroma_tuning;         /* A4 in Hz (ChromaParams::tuning); only read when freq_scale = SGX_FREQ_CHROMA */
    int32_t chroma_norm;          /* SGX_CHROMA_NORM_* */
} sgx_params;

/* Replaces StftPlan::new (:1204-1228), SpectrogramPlanner::{linear_plan :893-917, mel_plan :944-977}:
 * validates exactly like the reference constructors, builds window / twiddles / CSR filterbank on the
 * host in f64, casts to T and uploads.  On failure *out is NULL and sgx_last_create_error() has the text.
 * Every n_fft up to 2^20 (powers of two: 2^21) has a plan in both types, like the reference's planner (src/fft_backend.rs:372-389);
 * longer frames are SGX_BACKEND ("n_fft too large"). */
sgx_status sgx_plan_create(const sgx_params *params, sgx_plan **out);
void sgx_plan_destroy(sgx_plan *plan);

/* ---- constant-Q plans: SpectrogramPlanner::cqt_plan (src/spectrogram.rs:1127-1145), MappingKind::Cqt (:1785-1806, :1882-1904).
 * CqtParams (src/cqt.rs:17-165) flattened.  n_bins = bins_per_octave * n_octaves, f_k = f_min 2^(k / bins_per_octave).  Per bin
 * the kernel is K_k[j] = w[j] e^(+i 2 pi f_k j / sr), j < L_k = min(max(round(q sr / f_k), 1), n_fft) (round: half away from zero),
 * w = the symmetric window of length L_k; coefficients with |K| < sparsity_threshold * max|K| are zeroed; with `normalize` K is
 * multiplied by 1 / sqrt(sum |K|^2) when that sum is > 0 (src/cqt.rs:317-436).  A frame (unwindowed, same framing and centring as
 * the STFT) gives Y_k = sum_j T(Re K_k[j]) x[n_fft - L_k + j] + i sum_j T(-Im K_k[j]) x[n_fft - L_k + j] (src/cqt.rs:495-522);
 * the output is |Y_k|^2 -> amp_scale as for the other mappings, [batch][n_bins][n_frames].  The STFT window has no effect. */
typedef struct {
    uint32_t bins_per_octave, n_octaves;  /* both >= 1 */
    double f_min;                         /* finite and > 0 (NaN is refused, where the reference lets it through) */
    double q_factor;                      /* finite and > 0; CqtParams::new's default is 1 / (2^(1/bins_per_octave) - 1) */
    int32_t window_kind;                  /* SGX_WIN_* except SGX_WIN_CUSTOM (one custom window cannot have every length L_k) */
    double window_param;                  /* Kaiser beta / Gaussian std in samples */
    double sparsity_threshold;            /* values <= 0 (and NaN) disable the sparsity step */
    int32_t normalize;
} sgx_cqt_params;

/* params->freq_scale must be SGX_FREQ_CQT (sgx_plan_create refuses it); every sgx_params check of sgx_plan_create applies, the
 * mapping fields (n_mels, f_min, f_max, mel_norm, MFCC, ERB, chroma) are not read.  Refused: f_{n_bins-1} >= sr / 2 ("CQT maximum
 * frequency must be below Nyquist frequency"), SGX_AMP_COMPLEX, n_mfcc > 0.  sgx_execute, sgx_execute_timed, sgx_output_shape,
 * sgx_axes (frequencies f_k), sgx_reserve (forward) and sgx_shard_execute work as on a Mel plan; the FFT entry points (sgx_r2c,
 * sgx_c2r, sgx_istft) and sgx_mel_weights return SGX_INVALID_INPUT. */
sgx_status sgx_plan_create_cqt(const sgx_params *params, const sgx_cqt_params *cqt, sgx_plan **out);
/* ---- constant-Q transform: cqt() / CqtResult (src/cqt.rs:517-709), the complex coefficients on cqt()'s own framing.
 * For a signal of n samples cqt() takes klen = min(n, 16384) (:664), builds CqtKernel::generate(params, sr, klen) (:316-376: the
 * kernels of sgx_plan_create_cqt with n_fft = klen, except that the loop stops at the first bin with f_k >= sr / 2, :333-335, so
 * n_bins counts the bins below Nyquist) and applies them to the frames [f hop, f hop + klen), f < (n - klen) / hop + 1 (:671-675):
 * no centring, and hop > klen is legal.  Y_k of a frame is the sum of sgx_plan_create_cqt with n_fft = klen (:481-514).
 *   Read from params: n_fft (= klen, 1 .. 16384), hop_size (1 .. 2^24, not bound by n_fft), sample_rate_hz, amp_scale, dtype,
 *   device, has_log_params / floor_db; centre must be 0 and freq_scale SGX_FREQ_CQT.  amp_scale: SGX_AMP_COMPLEX gives Y itself,
 *   [batch][n_bins][n_frames] interleaved (re, im) in T as the complex STFT (CqtResult::data); POWER / MAGNITUDE / DECIBELS give
 *   re re + im im, its sqrt (CqtResult::to_power / to_magnitude, :591-612, each product and sum rounded in T) or its dB with the floor.
 *   Checks: those of sgx_plan_create_cqt less three — complex output, f_{n_bins-1} >= sr / 2 (the bins from the first such one on
 *   are dropped; SGX_INVALID_INPUT "no CQT bin lies below the Nyquist frequency" if none is left, where the reference is undefined)
 *   and hop_size <= n_fft.
 * The plan is a CQT plan: sgx_execute, sgx_execute_timed, sgx_output_shape, sgx_axes (the kept f_k; times f hop / sr), sgx_reserve,
 * sgx_cqt_kernels (the kept bins) and sgx_kernel_name serve it.  A caller who executes with n_samples < n_fft gets the STFT's one
 * zero-padded frame (sgx_output_shape), which is NOT cqt() of that signal: cqt() of a signal shorter than 16384 samples needs a
 * plan with n_fft = n_samples.
 * Calls whose signals hold one frame each (n_samples < n_fft + hop_size) run tiles of 16 signals ("cqt_mfma_rows") instead of one
 * tile per signal from a batch of 4096 on (measured: below that the per-signal tiles are faster until they run out of CUs); both
 * give the same bits.  sgx_kernel_name reports the route of the last call on such a plan. */
sgx_status sgx_plan_create_cqt_transform(const sgx_params *params, const sgx_cqt_params *cqt, sgx_plan **out);
/* Test entry: route = 0 automatic (above), 1 = per-signal tiles always, 2 = the rows tiles for every one-frame call (calls with
 * more frames keep the frame tiles).  SGX_INVALID_INPUT on any plan that is not a CQT transform
 * plan.  Reads no environment variable. */
sgx_status sgx_cqt_set_route(sgx_plan *plan, int32_t route);
/* The kernels as built (f64, before the cast to T), packed bin after bin: bin k's L_k values start at sum_{i<k} L_i.  Pass NULL
 * arrays to query `total` (= sum L_k) only; `lengths` has n_bins entries.  Works on host-only plans. */
sgx_status sgx_cqt_kernels(const sgx_plan *plan, size_t *total, uint32_t *lengths, double *re, double *im);

/* StftPlan::frame_count (:1230-1250) + SpectrogramPlan::output_shape (:512-519) */
sgx_status sgx_output_shape(const sgx_plan *plan, size_t n_samples, size_t *n_bins, size_t *n_frames);

/* The batched fast path replacing the per-signal loop `for s in signals { plan.compute(s) }`
 * (src/lib.rs:228-236) over SpectrogramPlan::compute (:240-294) / StftPlan::compute (:1424-1458).
 *   samples : batch rows of n_samples elements of T, row r at samples + r*sample_stride elements
 *   out     : [batch][n_bins][n_frames] row-major T (frames contiguous, S9); for SGX_AMP_COMPLEX
 *             interleaved (re,im) pairs, out_elems counts T elements (2 per complex value)
 *   out_elems != batch*n_bins*n_frames*(1|2)  ->  SGX_DIM_MISMATCH (compute_into, :423-434)
 *   mem_kind: SGX_MEM_HOST (plan-owned staging + copies, synchronous) or SGX_MEM_DEVICE
 *             (asynchronous on `hip_stream`, a hipStream_t; NULL = the null stream) */
sgx_status sgx_execute(sgx_plan *plan, const void *samples, size_t batch, size_t n_samples,
                       size_t sample_stride, void *out, size_t out_elems, int32_t mem_kind,
                       void *hip_stream);

/* Same as sgx_execute with device pointers, but launches `iters` times back-to-back between two
 * hipEvents recorded on `hip_stream` and returns the mean device time per launch in milliseconds
 * (used by bench.py for the roofline line).  Synchronises the stream. */
sgx_status sgx_execute_timed(sgx_plan *plan, const void *samples, size_t batch, size_t n_samples,
                             size_t sample_stride, void *out, size_t out_elems, void *hip_stream,
                             int32_t iters, float *ms_per_launch);

/* build_time_axis_seconds (:2128-2139), frequencies_hz (:1909-1931), mel_band_centres_hz (:2510-2530) */
sgx_status sgx_axes(const sgx_plan *plan, size_t n_frames, double *freqs /*n_bins*/, double *times /*n_frames*/);

/* Conforming per-call R2cPlan::process (src/fft_backend.rs:25-44, 423-431): host pointers, one frame,
 * in_len must be n_fft and out_len n_fft/2+1 complex values else SGX_DIM_MISMATCH (:264-282). */
sgx_status sgx_r2c(sgx_plan *plan, const void *in, size_t in_len, void *out, size_t out_len);

/* ---- inverse 1-D path ------------------------------------------------------------------------------------------
 * Conforming per-call C2rPlan::process (src/fft_backend.rs:526-565) = irfft (src/spectrogram.rs:4789-4811): host pointers,
 * in_len must be n_fft/2+1 complex values and out_len n_fft else SGX_DIM_MISMATCH; output scaled by 1/n_fft in T.  A
 * non-zero imaginary part in the DC (or, even n_fft, Nyquist) bin is ignored in the arithmetic and reported as
 * SGX_BACKEND after the output has been written — realfft's FftError::InputValues, mapped at :555-557. */
sgx_status sgx_c2r(sgx_plan *plan, const void *in, size_t in_len, void *out, size_t out_len);
/* istft (src/spectrogram.rs:4860-4946), batched over `batch` STFT matrices laid out [batch][n_bins][n_frames] complex T
 * (what sgx_execute writes for SGX_AMP_COMPLEX): per frame C2R, * window, overlap-add in ascending frame order,
 * / sum(w*w) where that exceeds T(1e-10), centre trim.  Uses the plan's n_fft / hop_size / window / centre.
 *   n_bins != n_fft/2+1 or out_elems != batch * sgx_istft_length  ->  SGX_DIM_MISMATCH
 *   mem_kind as sgx_execute; the DC/Nyquist check above is only reported for SGX_MEM_HOST (it needs a synchronisation). */
sgx_status sgx_istft_length(const sgx_plan *plan, size_t n_frames, size_t *n_samples);
sgx_status sgx_istft(sgx_plan *plan, const void *stft, size_t batch, size_t n_bins, size_t n_frames, void *out,
                     size_t out_elems, int32_t mem_kind, void *hip_stream);

/* make_window (:2159-2235): the plan's window coefficients as built (f64, before the cast to T). */
sgx_status sgx_window(const sgx_plan *plan, double *out /*n_fft*/);
/* build_mel_filterbank_matrix (:2302-2432) as CSR; pass NULL arrays to query nnz only. */
sgx_status sgx_mel_weights(const sgx_plan *plan, size_t *nnz, uint32_t *row_ptr /*n_mels+1*/,
                           uint32_t *cols, double *vals);

/* Pre-sizes the plan-owned scratch of the batched entry points for calls of up to `batch` signals of `n_samples` samples:
 * the MFCC plan's Mel-dB tensor always; with `inverse` the frame scratch of sgx_istft (generic path) for spectra of that many
 * frames; with `host_staging` the device staging of the SGX_MEM_HOST paths.  After it, such calls do not allocate
 * ("plans own scratch, no allocation in process", src/fft_backend.rs:21-24). */
sgx_status sgx_reserve(sgx_plan *plan, size_t batch, size_t n_samples, int32_t host_staging, int32_t inverse);

/* The HIP device ordinal the plan is bound to (resolved at creation when the params said -1); -2 for a host-only plan. */
int32_t sgx_plan_device(const sgx_plan *plan);

/* DimensionMismatch { expected, got } (src/error.rs:19-21, raised by validate_fft_io src/fft_backend.rs:264-282 and
 * compute_into src/spectrogram.rs:423-434): the two numbers of the plan's most recent SGX_DIM_MISMATCH. */
sgx_status sgx_last_dim_mismatch(const sgx_plan *plan, size_t *expected, size_t *got);

/* ---- multi-GPU (BASELINE config 4): utterances shard across ranks in contiguous blocks (remainder to the low
 * ranks), one process or thread per GPU, no data-path collective unless the caller asks for the gathered output. */
sgx_status sgx_shard_range(size_t batch, int32_t world_size, int32_t rank, size_t *start, size_t *count);

/* RCCL communicator, resolved at run time (the library does not link RCCL; a host that already carries one gets that copy).
 * sgx_comm_unique_id: rank 0 makes the 128-byte id and hands it to the other ranks by its own means (ncclGetUniqueId);
 * sgx_comm_create: ncclCommInitRank on `device` (-1 = current); collective over all ranks.
 * sgx_comm_adopt: wraps an ncclComm_t the host created itself (not destroyed by sgx_comm_destroy). */
#define SGX_COMM_ID_BYTES 128
typedef struct sgx_comm sgx_comm; /* opaque; one per rank */
sgx_status sgx_comm_unique_id(void *id128);
sgx_status sgx_comm_create(const void *id128, int32_t world_size, int32_t rank, int32_t device, sgx_comm **out);
sgx_status sgx_comm_adopt(void *nccl_comm, int32_t world_size, int32_t rank, int32_t device, sgx_comm **out);
void sgx_comm_destroy(sgx_comm *comm);
const char *sgx_comm_last_error(const sgx_comm *comm); /* NULL: the text of a failed create / adopt / unique_id */

/* All-gather of per-rank shards of `global_batch` items of `elems_per_item` elements (dtype SGX_F32 / SGX_F64; a complex value
 * counts as two): rank r contributes its sgx_shard_range block from `send`, every rank receives all blocks in rank order in
 * `recv` (device pointers; `send` may be the rank's own slice of `recv`).  Asynchronous on `hip_stream`.  Equal shards are one
 * ncclAllGather, ragged ones a group of ncclBroadcast. */
sgx_status sgx_gather(sgx_comm *comm, const void *send, void *recv, size_t global_batch, size_t elems_per_item, int32_t dtype,
                      void *hip_stream);

/* This rank's part of a `global_batch`-signal job: runs the plan on its shard (`shard_samples`: device pointer to the rank's
 * own sgx_shard_range block, rows `sample_stride` apart) into `shard_out` — or, if that is NULL, straight into its slice of
 * `gathered_out` — and, when `gathered_out` is not NULL, gathers all shards into it ([global_batch][n_bins][n_frames] on every
 * rank).  Asynchronous on `hip_stream`.  The plan and the communicator must be on the same device. */
sgx_status sgx_shard_execute(sgx_plan *plan, sgx_comm *comm, const void *shard_samples, size_t global_batch, size_t n_samples,
                             size_t sample_stride, void *shard_out, void *gathered_out, void *hip_stream);

/* The same, with the gather overlapped with the compute inside the call ("chunked and overlapped with compute"):
 * the shard is cut into `chunks` (1..64) runs of signals; while run k + 1 computes on `hip_stream`, run k's pieces of every rank
 * travel on a second stream owned by the communicator (a group of ncclBroadcast per run, each into the piece's own place in
 * `gathered_out`), ordered by events only.  `hip_stream` waits for the last exchange before the call's work counts as complete,
 * so the call is asynchronous on `hip_stream` like sgx_shard_execute.  chunks == 1 or gathered_out == NULL: sgx_shard_execute.
 * The result equals sgx_shard_execute's bit for bit.
 * EXPERIMENTAL: exercised on a stand-in RCCL at 2-3 ranks (tests/c_abi/shard_ranks.c) and on the real RCCL at ONE rank only; no run
 * on two or more real GPUs yet.  On any failure the two streams are re-joined before the call returns (the caller's stream waits
 * for whatever was queued on the exchange stream), but collectives other ranks have already issued for later runs stay pending:
 * after a non-OK status destroy the communicator (sgx_comm_destroy) on every rank. */
sgx_status sgx_shard_execute_chunked(sgx_plan *plan, sgx_comm *comm, const void *shard_samples, size_t global_batch,
                                     size_t n_samples, size_t sample_stride, void *shard_out, void *gathered_out, int32_t chunks,
                                     void *hip_stream);

/* ---- 2-D FFT path (BASELINE config 5): R2cPlan2d / C2rPlan2d (src/fft_backend.rs:169-246, 614-819), fft2d / ifft2d
 * (src/fft2d.rs:77-185), convolve_fft and the radial filters (src/image_ops.rs:80-432).  Batched: `batch` images of
 * nrows x ncols per call.  Real images are [batch][nrows][ncols] T; half spectra [batch][nrows][ncols/2+1] complex T
 * (interleaved).  The plan owns every intermediate buffer. */
typedef struct sgx_fft2d sgx_fft2d; /* opaque; same single-caller rule as sgx_plan */
sgx_status sgx_fft2d_create(size_t nrows, size_t ncols, int32_t dtype, int32_t device, sgx_fft2d **out);
void sgx_fft2d_destroy(sgx_fft2d *plan);
/* fft2d: unnormalised forward (rows R2C, then columns C2C) */
sgx_status sgx_fft2d_forward(sgx_fft2d *plan, const void *images, size_t batch, void *spectrum, int32_t mem_kind,
                             void *hip_stream);
/* ifft2d: columns inverse C2C, DC/Nyquist columns forced real, rows C2R, scale 1/(nrows*ncols) */
sgx_status sgx_fft2d_inverse(sgx_fft2d *plan, const void *spectrum, size_t batch, void *images, int32_t mem_kind,
                             void *hip_stream);
/* convolve_fft(image, kernel): kernel (krows x kcols, host pointer, T) is wrapped so its centre sits at (0,0)
 * (pad_kernel_for_fft, image_ops.rs:123-152), transformed once and multiplied into every image's spectrum.  The plan keeps
 * that spectrum on the device: a later call with the same kernel bytes and shape on the same stream reuses it (the kernel is
 * read from `kernel_host` during the call, never afterwards); sgx_fft2d_filter keeps its mask per (kind, cut-offs, stream).
 * f32 images with 1024 rows (the fused column stage): a kernel that is an outer product u v^T to f32 rounding (gaussian_kernel_2d is,
 * image_ops.rs:188-220) is multiplied in as the two 1-D spectra of u and v, and on 1024 x 1024 images its convolution runs as two
 * separable passes (rows, then columns) — the same linear operators as fft2d . product . ifft2d, within the f32 tolerance of the
 * general path.  Test switches, read at the call: SGX_CONV_RANK1=0 (every kernel through its full 2-D spectrum),
 * SGX_CONV_SEPARABLE=0 (rank-1 kernels through the three passes), SGX_SEP_GROUP=n (images per launch pair of the separable passes). */
sgx_status sgx_fft2d_convolve(sgx_fft2d *plan, const void *images, size_t batch, const void *kernel_host, size_t krows,
                              size_t kcols, void *out, int32_t mem_kind, void *hip_stream);
/* lowpass (kind 0, cut_lo), highpass (1, cut_lo), bandpass (2, cut_lo..cut_hi): binary radial masks built on the HALF
 * spectrum's own dimensions (image_ops.rs:236-267, 301-432 — the reference's quirk S14 is reproduced) */
sgx_status sgx_fft2d_filter(sgx_fft2d *plan, const void *images, size_t batch, int32_t kind, double cut_lo, double cut_hi,
                            void *out, int32_t mem_kind, void *hip_stream);
/* Pre-sizes the plan-owned intermediates (and, with `host_staging`, the device staging of the SGX_MEM_HOST paths) for calls of
 * up to `batch` images, so that those calls do not allocate. */
sgx_status sgx_fft2d_reserve(sgx_fft2d *plan, size_t batch, int32_t host_staging);
int32_t sgx_fft2d_device(const sgx_fft2d *plan); /* the HIP device ordinal the plan is bound to */
const char *sgx_fft2d_last_error(const sgx_fft2d *plan);
/* The route of the plan's last successful convolve / filter call (a failed call leaves it as it was): "separable" (rank-1 kernel,
 * 1024 x 1024 f32: two passes over pairs of real rows), "colconv_outer" / "colconv_spectrum" / "colconv_mask" (f32, 1024 rows: the
 * fused column kernel with a rank-1 kernel's two factors, a full kernel spectrum or a filter mask), each with "/chunked" when the
 * batch ran as chunks on two streams, "unfused" (separate forward, product and inverse passes), or "" before any such call. */
const char *sgx_fft2d_kernel_name(const sgx_fft2d *plan);

/* ---- 1-D complex-to-complex plan: C2cPlan<T> (src/fft_backend.rs:113-137; `Sample::plan_c2c`, src/sample.rs:61-66).  In
 * place, UNNORMALISED in both directions (the caller divides by n after an inverse, as the trait says), host pointers, `len`
 * complex values of T = n else SGX_DIM_MISMATCH.  Everything is allocated at creation. */
typedef struct sgx_c2c sgx_c2c; /* opaque; same single-caller rule as sgx_plan */
sgx_status sgx_c2c_create(size_t n, int32_t dtype, int32_t device, sgx_c2c **out);
void sgx_c2c_destroy(sgx_c2c *plan);
sgx_status sgx_c2c_forward(sgx_c2c *plan, void *buf, size_t len);
sgx_status sgx_c2c_inverse(sgx_c2c *plan, void *buf, size_t len);
const char *sgx_c2c_last_error(const sgx_c2c *plan);

/* ---- measurement utility ("verify the HBM peak on the box with a device memcpy / triad and quote the measured
 * peak next to the nominal"): streams `bytes` (0 = 1 GiB, four times the Infinity Cache) `iters` times with 16-byte accesses
 * from every CU and returns the rate in GB/s.  mode 0: copy (bytes read + bytes written per pass), 1: read only, 2: write only,
 * 3: one buffer read and two written per pass (the read : write mix of the linear-power STFT), counted as 3 x `bytes`.
 * Allocates and frees its own buffers on `device` (-1 = current); no plan involved, nothing on the transform path calls it. */
sgx_status sgx_membench(int32_t device, size_t bytes, int32_t mode, int32_t iters, double *gb_per_s);
/* The shader clock the device holds right now, in MHz: one wave per CU, enqueued on `hip_stream` behind whatever the caller has
 * launched there, counts shader cycles against the constant 100 MHz counter for ~20 us; the call waits for the stream and returns
 * the median over the CUs.  bench.py's `sustained` leg calls it between blocks of back-to-back launches (the clock a caller who
 * streams for seconds gets, next to the short timed region's). */
sgx_status sgx_clock_probe(int32_t device, void *hip_stream, double *mhz);

const char *sgx_last_error(const sgx_plan *plan);
const char *sgx_last_create_error(void);
/* Name of the kernel variant the plan dispatches to: the shape-specific kernels "r32x16_f32", "r32x32_f32", "r64x32_f32", "d512_f64", "d32x16_f64",
 * "d32x32_f64", or "reg_radix", "lds_radix2", "two_factor_dft", "bluestein", "direct_dft", or — frame lengths past the on-chip kernels, every n_fft up
 * to 2^20 (powers of two 2^21) — "big_four_step" / "big_chirpz" (transforms through global memory); CQT plans: "cqt_mfma_lds"
 * (the frames' samples staged in LDS) or "cqt_mfma_global" (spans too large for LDS) (a diagnostic: a call may step down this chain for
 * shapes the plan's kernel does not take). */
const char *sgx_kernel_name(const sgx_plan *plan);
/* Kernel of the plan's last successful sgx_execute / sgx_execute_timed call, "" before any: one of sgx_kernel_name's names, after the
 * call's own steps down the chain (a signal past a shape-specific kernel's 32-bit offsets runs on "reg_radix", a row past that kernel's on
 * "lds_radix2" / "two_factor_dft" / "direct_dft").  A diagnostic; a call in chunks reports its last chunk. */
const char *sgx_execute_kernel_name(const sgx_plan *plan);
/* Route of the plan's last successful sgx_istft / sgx_c2r call, "" before any: the fused inverse STFT kernels "istft1024c",
 * "istft2048", "istft_d512", "istft_d1024", "istft_reg", or rows into a frame scratch then the overlap-add, "c2r_reg+ola",
 * "c2r_chirpz+ola", "c2r_chirpz_half+ola", "c2r_rows+ola", "big+ola"; sgx_c2r: the same rows without "+ola". */
const char *sgx_istft_kernel_name(const sgx_plan *plan);
/* Filterbank stage (Mel / log-Hz / ERB / chroma rows, MFCC on top) of the plan's last successful sgx_execute / sgx_execute_timed call,
 * "" before any and for plans without a bank (a diagnostic, like sgx_kernel_name: the bank's shape decides which device code applies it).
 * In the launch sgx_kernel_name names: "r32x16_sched", "r32x16_sched_packed" (batches of short signals), "r32x16_sched512", "r32x16_sched_mfcc" (MFCC in the same launch), "r32x16_mfma",
 * "r32x16_csr", "r32x32_sched", "r64x32_sched", "d32x16_sched", "d512_sched", "d32x32_sched", "reg_radix_bands", "reg_radix_csr",
 * "generic_csr", "bluestein_rows"; "bank_rows": per-bin values from that launch, the rows in a second one.  A separate MFCC launch behind
 * the stage appends "+mfcc_acc" or "+mfcc_rows". */
const char *sgx_bank_stage_name(const sgx_plan *plan);
int32_t sgx_abi_version(void);
int32_t sgx_device_count(void);

/* ---- MDCT / IMDCT plans: MdctParams, mdct, imdct (src/mdct.rs:54-140, :387-497), batched.  window_size = 2N (even, >= 4), N
 * coefficients per frame, any hop >= 1; the window is make_window(window_kind, 2N) (a custom window must have 2N coefficients: the
 * reference panics there, this plan refuses it with SGX_INVALID_INPUT).  No centring and no padding: n_frames = (n_samples - 2N) / hop + 1,
 * fewer than 2N samples are SGX_INVALID_INPUT ("samples length (..) must be >= window_size (..)").
 *   forward  C[k, f] = sum_{n < 2N} x[f hop + n] w[n] cos(pi (2n + 1 + N)(2k + 1) / (4N)), k < N; out [batch][N][n_frames] T
 *   inverse  y_f[m] = (2/N) sum_k C[k, f] cos(pi (2m + 1 + N)(2k + 1) / (4N)), m < 2N, times w[m], added in ascending frame order into a
 *            zeroed [batch][hop n_frames + 2N - hop] T (no normalisation; zero frames: an empty output); n_coeffs != N is SGX_DIM_MISMATCH
 * Supported: every even window_size up to 8192 and the powers of two up to 16384, both types (larger: SGX_BACKEND).  out_elems must be
 * the exact element count (else SGX_DIM_MISMATCH); mem_kind and hip_stream as sgx_execute.  device -1: the current device, -2: a host-only
 * plan (validation, shapes, window, routes; the compute calls return SGX_BACKEND). */
typedef struct sgx_mdct sgx_mdct; /* opaque; same single-caller rule as sgx_fft2d / sgx_c2c */
sgx_status sgx_mdct_create(size_t window_size, size_t hop_size, int32_t window_kind, double window_param, const double *custom_window,
                           uint32_t custom_window_len, int32_t dtype, int32_t device, sgx_mdct **out);
void sgx_mdct_destroy(sgx_mdct *plan);
sgx_status sgx_mdct_output_shape(const sgx_mdct *plan, size_t n_samples, size_t *n_coeffs, size_t *n_frames);
sgx_status sgx_mdct_inverse_length(const sgx_mdct *plan, size_t n_frames, size_t *n_samples);
sgx_status sgx_mdct_forward(sgx_mdct *plan, const void *samples, size_t batch, size_t n_samples, void *out, size_t out_elems,
                            int32_t mem_kind, void *hip_stream);
sgx_status sgx_mdct_inverse(sgx_mdct *plan, const void *coeffs, size_t batch, size_t n_coeffs, size_t n_frames, void *out,
                            size_t out_elems, int32_t mem_kind, void *hip_stream);
/* Pre-sizes the plan-owned scratch (the generic route's chunk buffers; with host_staging the SGX_MEM_HOST staging) for forward calls of up
 * to `batch` signals of `n_samples` samples and inverse calls of as many frames, so that those calls do not allocate. */
sgx_status sgx_mdct_reserve(sgx_mdct *plan, size_t batch, size_t n_samples, int32_t host_staging);
sgx_status sgx_mdct_window(const sgx_mdct *plan, double *out /* window_size values, f64 as built */);
/* The route the plan runs in that direction: "k_mdct_fwd" (fused, N even with a register-tiled split of N/2), "k_imdct_ola" (fused, the
 * same lengths at hop == N), else "mdct_generic" / "imdct_generic" (fold, batched complex transform, post-twiddle, overlap-add). */
const char *sgx_mdct_kernel_name(const sgx_mdct *plan, int32_t inverse);
int32_t sgx_mdct_device(const sgx_mdct *plan);
const char *sgx_mdct_last_error(const sgx_mdct *plan); /* NULL plan: the text of the last failed create */

/* ---- binaural plans: compute_{itd,ipd,ild,ilr}_spectrogram (src/binaural.rs:472-560, :830-900, :1187-1240, :1530-1600), batched over
 * stereo pairs.  Each channel is the complex STFT (StftPlan::compute, src/spectrogram.rs:1424-1458) of the plan's STFT fields; with
 * bw = sample_rate / n_fft, start_bin = round(start_freq / bw) and stop_bin = round(end_freq / bw) (f64, half away from zero), the map is
 * [stop_bin - start_bin][n_frames] of, per bin k and frame (magphase :106-160 in T: mag = sqrt(fma(re, re, im im)), angle = atan2 of the
 * unit phase, mag 0 and angle 0 where fma(re, re, im im) == 0):
 *   ITD  pow(magL) + pow(magR) > 0 ? (np_mod(aL - aR + pi, 2 pi) - pi) / (2 pi bw k) : 0      (pow = magphase_power, :57-84)
 *   IPD  wrapped ? np_mod(aL - aR + pi, 2 pi) - pi : aL - aR
 *   ILD  magL + magR > 0 && magL > 0 && magR > 0 ? -20 log10(magR / magL) : NaN
 *   ILR  same condition, r = magR / magL: r < 1 ? 1 - r : -(1 - 1 / r); else NaN
 * with np_mod(x, m) = fmod(fmod(x, m) + m, m), in T. */
enum { SGX_BINAURAL_ITD = 0, SGX_BINAURAL_IPD = 1, SGX_BINAURAL_ILD = 2, SGX_BINAURAL_ILR = 3 };
typedef struct {
    int32_t kind;             /* SGX_BINAURAL_* */
    double start_freq;        /* Hz */
    double end_freq;          /* Hz */
    uint32_t magphase_power;  /* ITD: >= 1 (0 is SGX_INVALID_INPUT); read for validation only by the other kinds */
    int32_t wrapped;          /* IPD: wrap the difference to [-pi, pi) */
} sgx_binaural_params;
typedef struct sgx_binaural sgx_binaural; /* opaque; same single-caller rule as sgx_plan */

/* Only the STFT fields of `stft` are read (n_fft, hop_size, centre, window, sample_rate_hz, dtype, device); every sgx_plan_create check
 * applies to them, device -2 gives a host-only plan (validation, shapes, axes, route).  Then, word for word as ITDSpectrogramParams::new
 * (:410-460) and its siblings: "Start and end frequencies must be positive.", "Start frequency must be less than end frequency.", "End
 * frequency must be less than Nyquist frequency." (end > sr / 2).  Refused where the reference panics or computes with nonsense: a NaN
 * frequency ("Start and end frequencies must be finite."), magphase_power 0, an empty band stop_bin <= start_bin ("Frequency range should
 * have at least one bin").  On failure *out is NULL and sgx_binaural_last_error(NULL) has the text. */
sgx_status sgx_binaural_create(const sgx_params *stft, const sgx_binaural_params *params, sgx_binaural **out);
void sgx_binaural_destroy(sgx_binaural *plan);
/* start_bin, n_bins = stop_bin - start_bin, and the STFT's frame count for signals of n_samples samples */
sgx_status sgx_binaural_output_shape(const sgx_binaural *plan, size_t n_samples, size_t *start_bin, size_t *n_bins, size_t *n_frames);
/* frequencies bin * bw for the band's n_bins bins; times frame * hop / sample_rate (:541-553).  Either pointer may be NULL. */
sgx_status sgx_binaural_axes(const sgx_binaural *plan, size_t n_frames, double *freqs, double *times);
/* `batch` stereo pairs: left row r at left + r * sample_stride, right row r at right + r * sample_stride (elements of T), n_samples each;
 * out [batch][n_bins][n_frames] T.  out_elems must be that count (else SGX_DIM_MISMATCH); mem_kind and hip_stream as sgx_execute. */
sgx_status sgx_binaural_execute(sgx_binaural *plan, const void *left, const void *right, size_t batch, size_t n_samples, size_t sample_stride,
                                void *out, size_t out_elems, int32_t mem_kind, void *hip_stream);
/* The per-frame histograms of the Itd/Ipd/Ild/IlrSpectrogram::histogram methods (:323-370, :691-740, :1043-1090, :1385-1430) over maps
 * `values` [batch][n_bins][n_frames] T as sgx_binaural_execute writes them: out [batch][num_bins][n_frames] f64.  A value counts 1 into
 * bin min(floor((v - lo) / ((hi - lo) / num_bins)), num_bins - 1) (the cast saturates: NaN and negative quotients to 0) when it is finite
 * and lo <= v <= hi; then, per cell, powi(exponent) when exponent != 1 (ILD / ILR; 1 for ITD / IPD), then with `normalize` each column is
 * divided by its sum when that is > 0.  The counts are exact.  num_bins 1..32768. */
sgx_status sgx_binaural_histogram(sgx_binaural *plan, const void *values, size_t batch, size_t n_frames, size_t num_bins, double lo, double hi,
                                  int32_t exponent, int32_t normalize, double *out, size_t out_elems, int32_t mem_kind, void *hip_stream);
/* Pre-sizes the plan-owned scratch (the spectra of a chunk of pairs; with host_staging the SGX_MEM_HOST staging of sgx_binaural_execute)
 * for calls of up to `batch` pairs of `n_samples` samples, so that those calls do not allocate. */
sgx_status sgx_binaural_reserve(sgx_binaural *plan, size_t batch, size_t n_samples, int32_t host_staging);
/* The route: "r32x16_binaural_f32" (f32 n_fft 1024: both channels transformed and combined in one launch of the tuned kernel), else
 * "binaural_epilogue/<complex STFT route>" (the plan's complex STFT on each channel into scratch, then the epilogue kernel,
 * e.g. "binaural_epilogue/d32x16_f64"). */
const char *sgx_binaural_kernel_name(const sgx_binaural *plan);
int32_t sgx_binaural_device(const sgx_binaural *plan);
const char *sgx_binaural_last_error(const sgx_binaural *plan); /* NULL plan: the text of the last failed create */

/* ---- gammatone IIR plans: gammatone_iir_spectrogram / gammatone_center_frequencies (src/erb.rs:405-654), batched.  The time-domain
 * filter bank the reference offers beside the frequency-domain ErbFilterbank of the SGX_FREQ_ERB plans: no FFT, every (signal, frame,
 * band) is an 8th-order recurrence in f64 from zero state.
 *   centre frequencies cf[band], low to high: those of the SGX_FREQ_ERB plans for the same n_filters, f_min, f_max, erb_spacing
 *   per band, Ts = 1 / sample_rate, B = 1.019 2 pi (cf / 9.26449 + 24.7), th = 2 pi cf Ts, E = exp(-B Ts): four sections
 *     y = a0_k x + z0;  z0 = a1_k x + z1 - b1 y;  z1 = -b2 y      (Direct Form II transposed, a2 = 0, z0 = z1 = 0 at the frame's start)
 *     b1 = -2 cos(th) E, b2 = exp(-2 B Ts), a0_k = Ts, a1_k = -E (Ts cos(th) +- s Ts sin(th)) with +s2, -s2, +s1, -s1 for k = 1..4,
 *     s1 = sqrt(3 - 2 sqrt 2), s2 = sqrt(3 + 2 sqrt 2); a0_1 and a1_1 divided by the gain of iir_gain (:426-453)
 *   frames: no centring, no padding, n_frames = 1 + (n_samples - frame_size) / hop_size; frame f = samples [f hop, f hop + frame_size) as
 *     f64 times w[i] = 0.5 - 0.5 cos(2 pi i / (frame_size - 1))
 *   out[band][f] = T(sqrt(sum(y4^2) / frame_size)), the arithmetic in f64 for both T; with a dB floor, in T:
 *     v > eps ? 10 log10(v) : 10 log10(eps), eps = T(10^(db_floor / 10)) (a NaN value takes the floor, as T::max ignores it); the second
 *     value is computed once on the host.
 * Errors: sample_rate <= 0 "sample_rate must be > 0"; fewer than frame_size samples "signal is shorter than frame_size" (both
 * SGX_INVALID_INPUT, texts of the reference); the ErbParams::new checks on n_filters, f_min, f_max with their texts.  Refused where the
 * reference divides by zero or loops: frame_size < 2, hop_size == 0, a non-finite sample_rate or db_floor.  f_max above Nyquist is
 * accepted, as in the reference (the poles stay inside the unit circle).  Limits of the launch: n_filters <= 65536, frame_size and
 * hop_size below 2^31.  device -1: the current device, -2: a host-only plan (validation, shapes, centre frequencies, coefficients, route;
 * the compute calls return SGX_BACKEND). */
typedef struct sgx_gammatone sgx_gammatone; /* opaque; same single-caller rule as sgx_mdct */
#define SGX_GAMMATONE_COEFFS 11 /* doubles per band of sgx_gammatone_coefficients */
sgx_status sgx_gammatone_create(double sample_rate, size_t frame_size, size_t hop_size, uint32_t n_filters, double f_min, double f_max,
                                int32_t erb_spacing, int32_t has_db_floor, double db_floor, int32_t dtype, int32_t device,
                                sgx_gammatone **out);
void sgx_gammatone_destroy(sgx_gammatone *plan);
sgx_status sgx_gammatone_output_shape(const sgx_gammatone *plan, size_t n_samples, size_t *n_bands, size_t *n_frames);
/* `batch` signals: row r at samples + r * sample_stride (elements of T, sample_stride >= n_samples), n_samples each;
 * out [batch][n_bands][n_frames] T.  out_elems must be that count (else SGX_DIM_MISMATCH); mem_kind and hip_stream as sgx_execute. */
sgx_status sgx_gammatone_execute(sgx_gammatone *plan, const void *samples, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                                 size_t out_elems, int32_t mem_kind, void *hip_stream);
sgx_status sgx_gammatone_center_frequencies(const sgx_gammatone *plan, double *out /* n_filters */);
/* The coefficients as built (f64) and as the kernel reads them, per band: a0_1, a1_1 (both already divided by the gain), a0_2, a1_2,
 * a0_3, a1_3, a0_4, a1_4, b1, b2, gain. */
sgx_status sgx_gammatone_coefficients(const sgx_gammatone *plan, double *out /* [n_filters][SGX_GAMMATONE_COEFFS] */);
/* Pre-sizes the SGX_MEM_HOST staging for calls of up to `batch` signals of `n_samples` samples (the kernel itself needs no scratch). */
sgx_status sgx_gammatone_reserve(sgx_gammatone *plan, size_t batch, size_t n_samples, int32_t host_staging);
const char *sgx_gammatone_kernel_name(const sgx_gammatone *plan); /* "k_gammatone_iir": one kernel for every shape and both types */
int32_t sgx_gammatone_device(const sgx_gammatone *plan);
const char *sgx_gammatone_last_error(const sgx_gammatone *plan); /* NULL plan: the text of the last failed create */

/* ---- FIR plans: fft_convolve and OverlapSaveConvolver (src/convolution.rs:25-47, :149-270), batched overlap-save.  T = the plan's dtype,
 * everything is computed in T.  For row r, with L = taps - 1:
 *   y_r[n] = sum_{k < taps} h_r[k] x_r[n - k]
 * h is one impulse response for every row (ir_rows 1) or one per row (ir_rows = the batch of every call).  x_r[m] for m < 0 comes from
 * the row's history: the last L samples seen by earlier streaming calls, zeros after creation and after a reset.
 *   sgx_fir_process   streaming: n_out = n_samples; afterwards the history is the last L samples of (history | x), so a chunk shorter
 *                     than L shifts the old history and does not drop it.  Any cut of a signal into calls gives the samples of one
 *                     call, to rounding.  The history has `batch` rows, fixed by the first streaming call after creation or reset; a
 *                     later call with another batch is SGX_DIM_MISMATCH (expected / got in the text).
 *   sgx_fir_convolve  the full, stateless form: the history is taken as zero and left untouched, samples beyond n_samples are zero,
 *                     n_out = n_samples + taps - 1 (fft_convolve).
 * The reference ties its FFT size to the caller's block, next_power_of_two(block + taps - 1); a plan here picks its own segment
 * length P (sgx_fir_fft_size) and step S = P - L (sgx_fir_step) — block_size is a hint it records and the result does not depend on:
 *   route SGX_FIR_ROUTE_AUTO, taps <= 2049   "k_fir_os": P = next_power_of_two(4 taps) within 256 .. 4096, one fused launch
 *   otherwise (taps up to 2^19)              "fir_generic": P = next_power_of_two(2 taps), at least 256
 * The taps are rounded to T first; H = FFT_P(h) / P is built from them in f64 and rounded to T.  `out` must not overlap `x`.
 * Errors: "impulse response must not be empty" (taps 0; SGX_INVALID_INPUT, the reference's text); more than 2^19 taps SGX_BACKEND.
 * device -1: the current device, -2: a host-only plan (validation, shapes, route; the compute calls return SGX_BACKEND). */
typedef struct sgx_fir sgx_fir; /* opaque; same single-caller rule as sgx_mdct */
enum { SGX_FIR_ROUTE_AUTO = 0, SGX_FIR_ROUTE_GENERIC = 1 };
sgx_status sgx_fir_create(const double *ir /* [ir_rows][taps] */, size_t taps, size_t ir_rows, size_t block_size, int32_t route, int32_t dtype,
                          int32_t device, sgx_fir **out);
void sgx_fir_destroy(sgx_fir *plan);
/* `batch` rows: row r at x + r * sample_stride (elements of T, sample_stride >= n_samples), n_samples each; out [batch][n_out] T.
 * out_elems must be batch * n_out (else SGX_DIM_MISMATCH); mem_kind as sgx_execute, `stream` a hipStream_t as its hip_stream (the streams paragraph at the top). */
sgx_status sgx_fir_process(sgx_fir *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                           int32_t mem_kind, void *stream);
sgx_status sgx_fir_convolve(sgx_fir *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                            int32_t mem_kind, void *stream);
/* Zero history and no fixed row count again; the zeroing is enqueued on `stream`. */
sgx_status sgx_fir_reset(sgx_fir *plan, void *stream);
/* Pre-sizes the history for `batch` rows, the generic route's scratch for calls (either form) of up to `batch` rows of `n_samples`
 * samples and, with host_staging, the SGX_MEM_HOST staging, so that those calls do not allocate. */
sgx_status sgx_fir_reserve(sgx_fir *plan, size_t batch, size_t n_samples, int32_t host_staging);
size_t sgx_fir_fft_size(const sgx_fir *plan);
size_t sgx_fir_step(const sgx_fir *plan);
size_t sgx_fir_taps(const sgx_fir *plan);
const char *sgx_fir_kernel_name(const sgx_fir *plan); /* "k_fir_os" or "fir_generic" */
int32_t sgx_fir_device(const sgx_fir *plan);
const char *sgx_fir_last_error(const sgx_fir *plan); /* NULL plan: the text of the last failed create */

/* ---- deconvolution plans: fft_deconvolve (src/convolution.rs:60-106), batched.  Per row, with n = next_power_of_two(max(n_len, d_len))
 * and N, D the n-point real transforms of the zero-padded numerator and denominator (the library's R2C / C2R of that length, up to 2^20):
 *   eps = T(regularization) max_k |D_k|^2;   Q_k = N_k conj(D_k) / (|D_k|^2 + eps), exactly 0 where that denominator is 0;
 *   y = irfft_n(Q), truncated to n_len - d_len + 1 samples if n_len >= d_len, else to n_len (never below 1).
 * The denominator is one row for every numerator row (den_rows 1) or one per row (den_rows = batch). */
typedef struct sgx_deconv sgx_deconv; /* opaque; same single-caller rule as sgx_mdct */
sgx_status sgx_deconv_create(size_t n_len, size_t d_len, double regularization, int32_t dtype, int32_t device, sgx_deconv **out);
void sgx_deconv_destroy(sgx_deconv *plan);
size_t sgx_deconv_output_length(const sgx_deconv *plan);
/* numerator [batch][n_len], denominator [den_rows][d_len], out [batch][output_length] T, rows contiguous; batch <= 65535. */
sgx_status sgx_deconv_execute(sgx_deconv *plan, const void *numerator, const void *denominator, size_t batch, size_t den_rows, void *out,
                              size_t out_elems, int32_t mem_kind, void *stream);
sgx_status sgx_deconv_reserve(sgx_deconv *plan, size_t batch, size_t den_rows, int32_t host_staging);
int32_t sgx_deconv_device(const sgx_deconv *plan);
const char *sgx_deconv_last_error(const sgx_deconv *plan); /* NULL plan: the text of the last failed create */

/* ---- minimum-phase plans: minimum_phase / minimum_phase_with (src/min_phase.rs:55-141), batched.  The real-cepstrum method, per row,
 * with n = next_power_of_two(taps * max(oversample, 1)) (sgx_minphase_fft_size):
 *   H = FFT_n(h zero-padded);   eps = 1e-20 max_k |H_k|^2, or 1e-300 if that maximum is 0;   L_k = 0.5 ln(|H_k|^2 + eps);
 *   c = IFFT_n(L), folded: c_0 and c_{n/2} kept, c_1 .. c_{n/2-1} doubled, everything above n/2 dropped;
 *   C = FFT_n(folded c);   Hmin_k = exp(Re C_k) (cos Im C_k + i sin Im C_k);   y = Re IFFT_n(Hmin),
 * and the output row is its first sgx_minphase_output_length = min(out_len, n) samples.  minimum_phase is out_len = taps, oversample 8.
 * One deliberate difference from the reference, which computes in the sample type: the arithmetic is f64 for BOTH dtypes.  T = the
 * plan's dtype is the type of the input and output rows only; every transform, the log, the exp and the sin / cos are f64, and the
 * result is rounded to T once.  (In f32 the log amplifies the forward transform's rounding at every spectral null: on linear-phase
 * low-passes, the function's main input, an f32 pipeline is off by 5e-4 of the peak tap at 64 taps and by 0.6 at 4096.)
 *   route SGX_MINPHASE_ROUTE_AUTO, n <= 4096   "k_minphase": one launch, one workgroup per row, the row in LDS for all four transforms
 *   otherwise (n up to 2^20)                   "minphase_generic": the library's f64 R2C / C2R of length n (an internal plan, as the
 *                                              deconvolution plans) with elementwise kernels between them; SGX_MINPHASE_ROUTE_GENERIC
 *                                              asks for it at any n (the internal plans transform every n from 1 up: no lower limit)
 * Errors: "impulse response must not be empty" (taps 0), "out_len must be greater than zero" (both SGX_INVALID_INPUT, the reference's
 * texts); n above 2^20 SGX_BACKEND.  device -1: the current device, -2: a host-only plan (validation, shapes, route; compute and
 * reserve return SGX_BACKEND). */
typedef struct sgx_minphase sgx_minphase; /* opaque; same single-caller rule as sgx_mdct */
enum { SGX_MINPHASE_ROUTE_AUTO = 0, SGX_MINPHASE_ROUTE_GENERIC = 1 };
sgx_status sgx_minphase_create(size_t taps, size_t out_len, size_t oversample, int32_t route, int32_t dtype, int32_t device, sgx_minphase **out);
void sgx_minphase_destroy(sgx_minphase *plan);
/* ir [batch][taps] T, out [batch][output_length] T, rows contiguous; batch <= 65535; `out` must not overlap `ir`.  out_elems must be
 * batch * output_length (else SGX_DIM_MISMATCH); mem_kind as sgx_execute, `stream` a hipStream_t as its hip_stream (the streams
 * paragraph at the top holds for this call too: one operation of that stream, capturable once reserved). */
sgx_status sgx_minphase_execute(sgx_minphase *plan, const void *ir, size_t batch, void *out, size_t out_elems, int32_t mem_kind, void *stream);
/* Pre-sizes the generic route's scratch for calls of up to `batch` rows and, with host_staging, the SGX_MEM_HOST staging, so that
 * those calls do not allocate (the fused route needs no scratch). */
sgx_status sgx_minphase_reserve(sgx_minphase *plan, size_t batch, int32_t host_staging);
size_t sgx_minphase_fft_size(const sgx_minphase *plan);
size_t sgx_minphase_output_length(const sgx_minphase *plan);
size_t sgx_minphase_taps(const sgx_minphase *plan);
const char *sgx_minphase_kernel_name(const sgx_minphase *plan); /* "k_minphase" or "minphase_generic" */
int32_t sgx_minphase_device(const sgx_minphase *plan);
const char *sgx_minphase_last_error(const sgx_minphase *plan); /* NULL plan: the text of the last failed create */

/* ---- streaming spectrogram plans: the batched form of the SpectrogramPlan::compute_frame loop (src/spectrogram.rs:335-372,
 * python/examples/streaming.py) for signals that arrive in blocks.  A stream runs any plan sgx_plan_create accepts (every mapping,
 * amplitude scale, MFCC, window and both types; SGX_FREQ_CQT is SGX_INVALID_INPUT) on `batch` rows in lock step: every row gets the
 * same number of new samples in a call, and that number may change from call to call.  It carries the rows' pending samples on the
 * device; a call returns the frames that became complete, [batch][n_bins][f] T (complex: interleaved pairs, out_elems counts T).
 * Let pad = centre ? n_fft / 2 : 0.  The stream holds a pending run of p virtual samples per row, the same p for every row.
 *   after creation or sgx_stream_reset   p = pad (zeros), frames_emitted = 0, the row count is free
 *   sgx_stream_push of C >= 1 samples    P = p + C;  f = P >= n_fft ? (P - n_fft) / hop_size + 1 : 0;  the frames start at pending
 *                                        offsets 0, hop, .., (f - 1) hop;  afterwards p = P - f hop (0 <= p < n_fft).  f = 0 is legal:
 *                                        the block is staged, `out` is not touched (it may be NULL) and out_elems must be 0.
 *   sgx_stream_flush                     appends pad zeros and emits the frames that then fit.  A stream that has taken samples but
 *                                        emitted no frame since its reset (centre = 0 and fewer than n_fft samples in total) emits the
 *                                        reference's single zero-filled frame (frame_count :1239-1242); one that has taken no sample
 *                                        emits nothing.  Then the stream stands as after a reset, except that its row count stays fixed.
 * After the flush the frames of all calls, laid end to end, are the frames of sgx_execute of the same sgx_params on the whole signals:
 * the same count, the same order, equal to rounding.  Bit equality across different cuts of a signal is NOT promised: the frame count
 * of a call decides the launch shape, which may pick another variant of the transform.  The staging itself is exact: a push returns
 * the bits of the no-centre plan on the rows (pending | block).
 * The first push after creation or reset fixes the row count; a later push with another batch is SGX_DIM_MISMATCH (expected / got in
 * the text, as sgx_fir_process).  n_samples = 0 is SGX_INVALID_INPUT ("samples must be non-empty"); a wrong out_elems is
 * SGX_DIM_MISMATCH with the two numbers in sgx_stream_last_error.
 * A call is two launches: k_stream_stage (the pending samples and the new block into the second of two stream-owned work buffers, 16-byte
 * stores) and the plan's own launch on that buffer; sgx_stream_kernel_name is the sgx_kernel_name of the plan that runs the frames.
 * mem_kind as sgx_execute: SGX_MEM_HOST uses stream-owned staging and is synchronous, SGX_MEM_DEVICE is asynchronous on `stream` (a
 * hipStream_t) and is one operation of that stream; the stream's buffers are used in call order only, so calls that go to different
 * hipStreams must be ordered by the caller.  sgx_stream_reserve sizes the work buffers, the plan's scratch and (host_staging) the
 * staging for pushes of up to max_block samples on `batch` rows and the flush behind them: such calls allocate nothing and do not
 * synchronise; a larger one replaces a work buffer once (it waits for `stream` and the device).  It needs a stream without pending
 * samples of earlier pushes (after creation, reset or flush).  device -1: the current device, -2: a host-only stream (validation and
 * the bookkeeping below; push, flush and reserve return SGX_BACKEND). */
typedef struct sgx_stream sgx_stream; /* opaque; same single-caller rule as sgx_fir */
sgx_status sgx_stream_create(const sgx_params *params, sgx_stream **out);
void sgx_stream_destroy(sgx_stream *s);
/* Pure bookkeeping (host-only streams too): one push of n_samples onto `pending` gives n_frames and leaves pending_after. */
sgx_status sgx_stream_step(const sgx_stream *s, size_t pending, size_t n_samples, size_t *n_frames, size_t *pending_after);
size_t sgx_stream_pending(const sgx_stream *s);        /* p */
size_t sgx_stream_frames_emitted(const sgx_stream *s); /* since creation / reset / flush */
sgx_status sgx_stream_flush_frames(const sgx_stream *s, size_t *n_frames); /* what sgx_stream_flush would emit now */
size_t sgx_stream_n_bins(const sgx_stream *s);
/* row r at x + r * sample_stride (elements of T, sample_stride >= n_samples); out_elems = batch * n_bins * f (* 2 for complex) */
sgx_status sgx_stream_push(sgx_stream *s, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                           int32_t mem_kind, void *stream);
sgx_status sgx_stream_flush(sgx_stream *s, void *out, size_t out_elems, int32_t mem_kind, void *stream);
/* The zeros after a reset are not read from memory, so nothing is enqueued on `stream`. */
sgx_status sgx_stream_reset(sgx_stream *s, void *stream);
sgx_status sgx_stream_reserve(sgx_stream *s, size_t batch, size_t max_block, int32_t host_staging);
/* A diagnostic: how many times the stream has allocated or replaced one of its own buffers (work buffers, host staging) so far.  It
 * does not move across calls that fit what was reserved. */
size_t sgx_stream_allocations(const sgx_stream *s);
const char *sgx_stream_kernel_name(const sgx_stream *s);
int32_t sgx_stream_device(const sgx_stream *s);
const char *sgx_stream_last_error(const sgx_stream *s); /* NULL: the text of the last failed create */

/* ---- streaming inverse STFT plans: istft (src/spectrogram.rs:4860-4946) for frames that arrive in runs — the synthesis half of an
 * analysis -> modify -> synthesis loop on live audio (python/examples/streaming.py).  A stream reads n_fft / hop_size / window /
 * centre / dtype / device of sgx_params as sgx_istft does (every check of sgx_plan_create applies; SGX_FREQ_CQT is
 * SGX_INVALID_INPUT) and runs `batch` rows in lock step: every row gets the same number f >= 1 of new frames in a call, and f may
 * change from call to call.  A call returns the samples that no later frame can change; the unfinished overlap tail stays on the
 * device.  Let pad = centre ? n_fft / 2 : 0; positions are those of the untrimmed signal; F = the frames taken since creation, reset
 * or flush; E(F) = (F - 1) hop_size + n_fft.
 *   hi(F) = max(pad, min(F hop_size, E(F) - pad)),  hi(0) = pad
 *   sgx_istream_push of f frames   returns positions [hi(F), hi(F + f)) of every row, [batch][m] T; m = 0 is legal: `out` is not
 *                                  touched (it may be NULL) and out_elems must be 0
 *   sgx_istream_flush              returns [hi(F), E(F) - pad).  The one exception is the reference's quirk (:4933-4941): centre, even
 *                                  n_fft and exactly one frame in total give the whole untrimmed frame [0, n_fft).  A stream that has
 *                                  taken no frame emits nothing.  Then the stream stands as after a reset, except that its row count
 *                                  stays fixed.
 * After the flush the samples of all calls, laid end to end, are those of sgx_istft on all frames at once: sgx_istft_length(F)
 * samples, the same order, equal to rounding.  Bit equality with sgx_istft, or across different cuts, is NOT promised (the rows'
 * launcher may choose by row count, the paired routes pair the frames of a call, sgx_istft may take a fused kernel).  The arithmetic
 * per sample is that of sgx_istft's unfused route: the windowed row values of the covering frames added in ascending frame order,
 * divided by the sum of the rounded w w over all covering frames where that exceeds 1e-10; the carry holds raw partial sums only.
 * The imaginary parts of the DC bin, and of the Nyquist bin at even n_fft, are ignored on both memory kinds and not reported.
 * `spec` is [batch][n_bins][bin_stride] complex T (interleaved pairs), frame j of bin k of row b at b n_bins bin_stride + k bin_stride
 * + j: bin_stride = n_frames is a dense matrix, a larger one a run of frames inside a wider resident matrix (SGX_MEM_DEVICE only;
 * SGX_MEM_HOST needs bin_stride == n_frames).  n_bins != n_fft / 2 + 1 or a wrong out_elems is SGX_DIM_MISMATCH with the two numbers
 * in sgx_istream_last_error; n_frames = 0 is SGX_INVALID_INPUT.  The first push after creation or reset fixes the row count; a later
 * push with another batch is SGX_DIM_MISMATCH (text as sgx_stream_push).  A failed call moves no state.
 * A call is two launches: the rows of sgx_istft's unfused route into a stream-owned frame scratch, and k_istream_ola (carry + new
 * frames -> `out` and the second of two stream-owned carry buffers of n_fft T per row).  SGX_MEM_HOST uses stream-owned staging and is
 * synchronous, SGX_MEM_DEVICE is asynchronous on `stream` (a hipStream_t) and is one operation of that stream; calls that go to
 * different hipStreams must be ordered by the caller.  sgx_istream_reserve sizes the carry buffers, the frame scratch and
 * (host_staging) the staging for pushes of up to max_frames frames on `batch` rows and the flush behind them: such calls allocate
 * nothing and do not synchronise; a larger one replaces a buffer once (it waits for `stream` and the device).  It needs a stream
 * that carries nothing (after creation, reset or flush).  device -1: the current device, -2: a host-only stream (validation and the
 * bookkeeping below; push, a flush with frames taken, and reserve return SGX_BACKEND). */
typedef struct sgx_istream sgx_istream; /* opaque; same single-caller rule as sgx_fir */
sgx_status sgx_istream_create(const sgx_params *params, sgx_istream **out);
void sgx_istream_destroy(sgx_istream *s);
/* Pure bookkeeping (host-only streams too): the samples per row a push of n_frames frames returns on a stream that has taken
 * frames_taken; n_frames = 0 asks for the flush after frames_taken frames instead. */
sgx_status sgx_istream_step(const sgx_istream *s, size_t frames_taken, size_t n_frames, size_t *n_samples);
size_t sgx_istream_frames_taken(const sgx_istream *s);    /* F */
size_t sgx_istream_samples_emitted(const sgx_istream *s); /* per row, since creation / reset / flush */
size_t sgx_istream_pending(const sgx_istream *s);         /* samples carried per row, <= n_fft */
sgx_status sgx_istream_flush_samples(const sgx_istream *s, size_t *n_samples); /* what sgx_istream_flush would return now, per row */
/* out_elems = batch * m */
sgx_status sgx_istream_push(sgx_istream *s, const void *spec, size_t batch, size_t n_bins, size_t n_frames, size_t bin_stride, void *out,
                            size_t out_elems, int32_t mem_kind, void *stream);
sgx_status sgx_istream_flush(sgx_istream *s, void *out, size_t out_elems, int32_t mem_kind, void *stream);
/* A dropped carry is never read again, so nothing is enqueued on `stream`. */
sgx_status sgx_istream_reset(sgx_istream *s, void *stream);
sgx_status sgx_istream_reserve(sgx_istream *s, size_t batch, size_t max_frames, int32_t host_staging);
/* A diagnostic: how many times the stream has allocated or replaced one of its own buffers (carry, frame scratch, host staging). */
size_t sgx_istream_allocations(const sgx_istream *s);
/* the rows' route of the last call + "+stream_ola", e.g. "c2r_reg+stream_ola"; "" before any call */
const char *sgx_istream_kernel_name(const sgx_istream *s);
int32_t sgx_istream_device(const sgx_istream *s);
const char *sgx_istream_last_error(const sgx_istream *s); /* NULL: the text of the last failed create */

/* ---- sample-rate conversion plans: batched band-limited resampling with torchaudio.functional.resample's semantics (the reference
 * has no resampler; this is the step in front of every plan above when the audio is not at the plan's rate).  Rates are positive
 * integers; g = gcd(orig_freq, new_freq), M = orig_freq / g (sgx_resample_down), L = new_freq / g (sgx_resample_up), base = min(L, M) rolloff.
 *   phi(t) = sinc(t) w(t / lpw) for |t| < lpw, 0 otherwise; sinc(t) = sin(pi t) / (pi t), sinc(0) = 1; lpw = lowpass_filter_width
 *   w(u)   = cos^2(pi u / 2) (SGX_RESAMPLE_SINC_HANN) or I0(beta sqrt(1 - u^2)) / I0(beta) (SGX_RESAMPLE_SINC_KAISER)
 *   y[m]   = (base / M) sum_n x[n] phi(base (n / M - m / L)),  0 <= m < ceil(n_samples L / M),  x = 0 outside [0, n_samples)
 * Polyphase form, m = q L + p with 0 <= p < L:  y[q L + p] = sum_{k < K} c[p][k] x[q M + j0(p) + k], where j0(p) is the smallest j with
 * |base (j / M - p / L)| < lpw (sgx_resample_phase_offsets), K the largest number of such j over p (sgx_resample_taps_per_phase) and
 * c[p][k] = (base / M) phi(base ((j0(p) + k) / M - p / L)), exactly 0 beyond the support (sgx_resample_taps).  The table is built in f64,
 * rounded once to T and uploaded.  Equal rates (M = L = 1) are the identity: K = 1, c = [[1]], j0 = [0].
 * Arithmetic: every output is one chain in T, acc = 0, then acc = fma(c[p][k], x[..], acc) for k = 0 .. K - 1 ascending, on both routes.
 * The bits of an output therefore depend neither on the route nor on the tiling nor on how a stream is cut into calls, and an output
 * whose K samples are all zero is exactly zero.
 *   sgx_resample_resample   stateless, whole rows: out [batch][sgx_resample_out_len(n_samples)].
 *   sgx_resample_process    streaming: `batch` rows in lock step, n_samples >= 1 new samples per row; returns every output whose whole
 *                           window is known and that no earlier call returned.  With N = the samples consumed so far (sgx_resample_consumed)
 *                           and E = the outputs emitted (sgx_resample_emitted), after the call E = #{ m : floor(m / L) M + j0(m mod L)
 *                           + K - 1 <= N - 1 }; the count is what sgx_resample_step says, it may be 0 (`out` may then be NULL, out_elems 0).
 *                           The first call after creation, reset or flush fixes the row count; another batch is SGX_DIM_MISMATCH
 *                           (expected / got in the text) and moves no state.
 *   sgx_resample_flush      takes the future as zeros and returns the outputs E .. ceil(N L / M) - 1 of every row; then the plan
 *                           stands as after sgx_resample_reset.  Without a call to sgx_resample_process before it, it returns nothing.
 * After the flush the outputs of all calls, laid end to end, are bit for bit those of sgx_resample_resample on the whole rows.
 *   route SGX_RESAMPLE_ROUTE_AUTO, K <= 64, L <= 512 and a tile within 64 KiB of LDS   "k_resample_pp": one fused launch, samples in
 *                           LDS, a work item's coefficients in registers; sgx_resample_tile outputs per workgroup tile
 *   otherwise               "resample_generic": table and samples from global memory; L K above 2^22 coefficients is
 *                           SGX_INVALID_INPUT, the text names the reduced ratio M : L
 * The device holds each row's last K - 1 samples in one of two plan-owned buffers; the next history is written into the other one and
 * copied back on `stream`, so no launch reads what it writes.  Rows: row r at x + r * sample_stride (elements of T, sample_stride >=
 * n_samples); `out` must not overlap `x`; out_elems must be batch * n_out (else SGX_DIM_MISMATCH); mem_kind as sgx_execute, `stream`
 * a hipStream_t as its hip_stream (the streams paragraph at the top: a device-pointer call is one operation of `stream`, allocates
 * nothing within what sgx_resample_reserve sized — the device path of sgx_resample_resample never allocates — and can be captured).
 * Errors (SGX_INVALID_INPUT): rates <= 0, lowpass_filter_width < 1, rolloff outside (0, 1], an unknown method or route, beta not
 * finite or < 0 (Kaiser).  device -1: the current device, -2: a host-only plan (the table and every accessor below; the compute calls
 * and reserve return SGX_BACKEND). */
typedef struct sgx_resample sgx_resample; /* opaque; same single-caller rule as sgx_fir */
enum { SGX_RESAMPLE_SINC_HANN = 0, SGX_RESAMPLE_SINC_KAISER = 1 };
enum { SGX_RESAMPLE_ROUTE_AUTO = 0, SGX_RESAMPLE_ROUTE_GENERIC = 1 };
sgx_status sgx_resample_create(int64_t orig_freq, int64_t new_freq, int32_t lowpass_filter_width, double rolloff, int32_t method, double beta,
                               int32_t route, int32_t dtype, int32_t device, sgx_resample **out);
void sgx_resample_destroy(sgx_resample *plan);
sgx_status sgx_resample_resample(sgx_resample *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                                 size_t out_elems, int32_t mem_kind, void *stream);
sgx_status sgx_resample_process(sgx_resample *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                                size_t out_elems, int32_t mem_kind, void *stream);
sgx_status sgx_resample_flush(sgx_resample *plan, void *out, size_t out_elems, int32_t mem_kind, void *stream);
/* Zero history, nothing consumed and no fixed row count again; the zeroing is enqueued on `stream`. */
sgx_status sgx_resample_reset(sgx_resample *plan, void *stream);
/* Pre-sizes the history for `batch` rows and, with host_staging, the SGX_MEM_HOST staging for calls of up to max_block samples per row,
 * so that those calls and the flush behind them do not allocate. */
sgx_status sgx_resample_reserve(sgx_resample *plan, size_t batch, size_t max_block, int32_t host_staging);
/* Pure arithmetic (host-only plans too): the outputs per row a call of n_samples samples returns on a stream that has consumed
 * `consumed`, and what it has consumed afterwards (may be NULL); n_samples = 0 asks for the flush after `consumed` samples instead. */
sgx_status sgx_resample_step(const sgx_resample *plan, size_t consumed, size_t n_samples, size_t *n_out, size_t *consumed_after);
size_t sgx_resample_out_len(const sgx_resample *plan, size_t n_samples); /* ceil(n_samples L / M) */
size_t sgx_resample_up(const sgx_resample *plan);                        /* L */
size_t sgx_resample_down(const sgx_resample *plan);                      /* M */
size_t sgx_resample_taps_per_phase(const sgx_resample *plan);            /* K */
sgx_status sgx_resample_taps(const sgx_resample *plan, double *taps /* [L][K]: the T-valued coefficients */);
sgx_status sgx_resample_phase_offsets(const sgx_resample *plan, int64_t *offsets /* [L]: j0(p) */);
size_t sgx_resample_tile(const sgx_resample *plan);      /* outputs per workgroup tile of "k_resample_pp"; 0 on the generic route */
size_t sgx_resample_consumed(const sgx_resample *plan);  /* N, per row, since creation / reset / flush */
size_t sgx_resample_emitted(const sgx_resample *plan);   /* E */
/* A diagnostic: how many times the plan has allocated or replaced one of its own buffers (history, host staging). */
size_t sgx_resample_allocations(const sgx_resample *plan);
const char *sgx_resample_kernel_name(const sgx_resample *plan); /* "k_resample_pp" or "resample_generic" */
int32_t sgx_resample_device(const sgx_resample *plan);
const char *sgx_resample_last_error(const sgx_resample *plan); /* NULL plan: the text of the last failed create */

/* ---- Welch plans: batched spectrum estimates of whole signals — the averaged periodogram (PSD), the cross-spectral density of two
 * signals (CSD) and their magnitude-squared coherence — with the semantics of scipy.signal.welch / csd / coherence for real input
 * (nfft = nperseg = n_fft, noverlap = n_fft - hop_size, average = "mean", one-sided).  The reference has no such estimate; every
 * forward plan above ends in a [bins][frames] map.
 *   segments  s = 0 .. m - 1 hold the samples [s hop, s hop + n_fft), m = 1 + (n_samples - n_fft) / hop (sgx_welch_n_segments): no
 *             padding (params->centre must be 0), a tail that fills no segment is ignored; n_samples < n_fft is SGX_DIM_MISMATCH
 *             (scipy shrinks the segment instead)
 *   X_s       = FFT(w (x_s - trend_s)): the detrend comes first — nothing, the segment's mean, or its least-squares line — then the
 *             window (any window of sgx_params, custom tables included; SGX_WIN_HANNING is the symmetric Hann, scipy's "hann" string
 *             the periodic one)
 *   PSD       Pxx[k] = g_k scale mean_s |X_s[k]|^2                  out [batch][n_bins] T
 *   CSD       Pxy[k] = g_k scale mean_s conj(X_s[k]) Y_s[k]         out [batch][n_bins] interleaved (re, im) pairs of T
 *   COHERENCE C[k]   = |Pxy[k]|^2 / (Pxx[k] Pyy[k])                 out [batch][n_bins] T; all three sums come from one pass
 *   g_k = 2 except g_0 = 1 and, for even n_fft, g_{n_fft/2} = 1; scale = 1 / (sample_rate sum w^2) for SGX_WELCH_DENSITY and
 *   1 / (sum w)^2 for SGX_WELCH_SPECTRUM, computed in f64 on the host (sgx_welch_scale).
 * Routes: "k_welch" (SGX_WELCH_ROUTE_AUTO, n_fft a power of two 256 .. 4096): one fused launch that keeps the running sums on chip and
 * stores no segment's spectrum — a workgroup takes a tile of sgx_welch_tile consecutive segments of one row and leaves one partial in
 * plan scratch, a second small launch adds a row's partials in tile order; "welch_generic" (every other n_fft an sgx_plan accepts,
 * and any n_fft with SGX_WELCH_ROUTE_GENERIC): segments gathered to scratch, transformed by an internal plan and added in segment
 * order, over chunks of at most max_scratch_bytes per buffer (0: 256 MiB).  Neither route uses atomics: a row's result is the same
 * bits whatever the batch size, the row's place in the batch and the number of calls; on the generic route also whatever the chunk size.
 * conj(X) X is formed unfused, so the CSD of a signal with itself has a zero imaginary part and the PSD's bits as its real part, and
 * swapping x and y conjugates the CSD bit for bit.
 * Rows: row r at x + r * sample_stride (y likewise; elements of T, sample_stride >= n_samples); y must be NULL for a PSD plan and
 * non-NULL otherwise (SGX_INVALID_INPUT); out_elems must be batch * n_bins (CSD: twice that) else SGX_DIM_MISMATCH; mem_kind as
 * sgx_execute, `stream` a hipStream_t as its hip_stream.  Not offered: average = "median", zero padding to nfft > nperseg, two-sided
 * or complex input, sums carried across calls.
 * Errors (SGX_INVALID_INPUT): centre != 0, an unknown kind, detrend, scaling or route, and every STFT check of sgx_plan_create
 * (n_fft, hop_size in 1 .. n_fft, the window, the sample rate).  device -1: the current device, -2: a host-only plan (every accessor
 * below; execute and reserve return SGX_BACKEND behind their shape checks). */
typedef struct sgx_welch sgx_welch; /* opaque; same single-caller rule as sgx_fir */
enum { SGX_WELCH_PSD = 0, SGX_WELCH_CSD = 1, SGX_WELCH_COHERENCE = 2 };
enum { SGX_WELCH_DETREND_NONE = 0, SGX_WELCH_DETREND_CONSTANT = 1, SGX_WELCH_DETREND_LINEAR = 2 };
enum { SGX_WELCH_DENSITY = 0, SGX_WELCH_SPECTRUM = 1 };
enum { SGX_WELCH_ROUTE_AUTO = 0, SGX_WELCH_ROUTE_GENERIC = 1 };
/* Reads n_fft, hop_size, centre, the window fields, sample_rate_hz, dtype and device of `params`. */
sgx_status sgx_welch_create(const sgx_params *params, int32_t kind, int32_t detrend, int32_t scaling, int32_t route, size_t max_scratch_bytes,
                            sgx_welch **out);
void sgx_welch_destroy(sgx_welch *plan);
size_t sgx_welch_n_bins(const sgx_welch *plan);                        /* n_fft / 2 + 1 */
size_t sgx_welch_n_segments(const sgx_welch *plan, size_t n_samples);  /* m; 0 when n_samples < n_fft */
sgx_status sgx_welch_frequencies(const sgx_welch *plan, double *freqs /* [n_bins]: k sample_rate / n_fft */);
sgx_status sgx_welch_window(const sgx_welch *plan, double *window /* [n_fft]: as built in f64, before the cast to T */);
double sgx_welch_scale(const sgx_welch *plan);                         /* the f64 factor `scale` above */
sgx_status sgx_welch_execute(sgx_welch *plan, const void *x, const void *y, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                             size_t out_elems, int32_t mem_kind, void *stream);
/* Pre-sizes the partials (generic route: the chunk's scratch and the internal plan's) and, with host_staging, the SGX_MEM_HOST staging
 * for calls of up to `batch` rows of n_samples samples, so that those calls do not allocate. */
sgx_status sgx_welch_reserve(sgx_welch *plan, size_t batch, size_t n_samples, int32_t host_staging);
/* A diagnostic: how many times the plan has allocated or replaced one of its own buffers. */
size_t sgx_welch_allocations(const sgx_welch *plan);
size_t sgx_welch_tile(const sgx_welch *plan);             /* segments per workgroup tile of "k_welch"; 0 on the generic route */
const char *sgx_welch_kernel_name(const sgx_welch *plan); /* "k_welch" or "welch_generic" */
int32_t sgx_welch_device(const sgx_welch *plan);
const char *sgx_welch_last_error(const sgx_welch *plan); /* NULL plan: the text of the last failed create */

/* ---- Kaldi plans: batched Kaldi-compatible filterbank (fbank) and MFCC features of whole signals, with the semantics of
 * torchaudio.compliance.kaldi.fbank / .mfcc for dither = 0 and vtln_warp = 1, one row per batch item.  sgx_params cannot express them:
 * a frame shorter than the transform, per-frame mean removal and pre-emphasis before the window, triangles on Kaldi's mel scale, the
 * natural log and a frames x features layout.
 *   sizes     N = int(fs frame_length_ms / 1000) (window_size), shift = int(fs frame_shift_ms / 1000) (window_shift), P = the next power
 *             of two >= N with round_to_power_of_two, else N (padded_window_size)
 *   frames    snip_edges != 0: m = 1 + (n - N) / shift, frame t starts at t shift.  snip_edges == 0: m = (n + shift / 2) / shift, frame t
 *             starts at t shift + shift / 2 - N / 2 and the row is mirrored at both ends: index i < 0 reads x[-i - 1], i >= n reads
 *             x[2 n - 1 - i].  n < N is SGX_DIM_MISMATCH in both modes (torchaudio returns an empty matrix)
 *   per frame 1. remove_dc_offset: subtract the frame's mean;  2. raw_energy: the log energy, log(max(sum f^2, eps_T)), then
 *             max(., log(energy_floor)) when energy_floor > 0;  3. preemphasis_coefficient a != 0: f[j] - a f[j - 1] with f[-1] := f[0];
 *             4. the window;  5. the log energy here when raw_energy == 0;  6. zero-pad to P, real FFT;  7. |X|, squared with use_power.
 *             The mean leaves the samples before the difference and the window; it is not folded into a later term
 *   windows   with a = 2 pi / (N - 1): hanning 0.5 - 0.5 cos(a j); hamming 0.54 - 0.46 cos(a j); povey hanning^0.85; rectangular;
 *             blackman c - 0.5 cos(a j) + (0.5 - c) cos(2 a j), c = blackman_coeff
 *   bank      num_mel_bins x (P / 2 + 1), the last column (Nyquist) zero; high_freq <= 0 means high_freq + fs / 2;
 *             mel(f) = 1127 ln(1 + f / 700); band b has left, centre, right at mel(low) + (b, b + 1, b + 2) delta,
 *             delta = (mel(high) - mel(low)) / (bins + 1); the weight at bin k < P / 2 is
 *             max(0, min((mel(k fs / P) - l) / (c - l), (r - mel(k fs / P)) / (r - c)))
 *   fbank     E = spectrum . bank^T; with use_log_fbank log(max(E, eps_T)); eps_T = 2^-23 (f32) or 2^-52 (f64).  use_energy adds the
 *             log energy as a column: first, or last with htk_compat.  n_out = num_mel_bins (+ 1)
 *   MFCC      num_ceps > 0: the log-power fbank (use_power and use_log_fbank are not read) times the first num_ceps rows of the
 *             orthonormal DCT-II, D[i][b] = s_i sqrt(2 / B) cos(pi / B (b + 1/2) i), s_0 = 1 / sqrt 2, times the lifter
 *             1 + Q / 2 sin(pi i / Q) when Q = cepstral_lifter != 0; use_energy replaces C0 with the log energy, htk_compat moves C0
 *             to the last column.  n_out = num_ceps
 *   subtract_mean  subtracts each column's mean over the row's frames
 *   out       [batch][m][n_out] T: frames x features, as Kaldi lays them out
 * Every maximum keeps a NaN: a frame that holds a non-finite sample is non-finite in every feature and no other frame is.
 * The tables are built in extended precision on the host, rounded once to f64 (the accessors below) and cast to T; torchaudio builds
 * them in f32.
 * Routes: "k_kaldi" (SGX_KALDI_ROUTE_AUTO, P = 256, 512, 1024 or 2048 and at most 256 bands): one fused launch — a workgroup takes a
 * tile of sgx_kaldi_tile consecutive frames of one row, preprocesses and transforms them on chip and stores nothing but the features;
 * "kaldi_generic" (every other P up to 2^20, and any P with SGX_KALDI_ROUTE_GENERIC): frames gathered to scratch, transformed by an
 * internal plan, then bank, log, DCT and energy, over chunks of at most max_scratch_bytes per buffer (0: 256 MiB).  subtract_mean is
 * one more small launch that adds a row's frames in frame order.  No route uses atomics: a row's result is the same bits whatever the
 * batch size, the row's place in the batch, the number of calls and, on the generic route, the chunk size.
 * Rows: row r at x + r * sample_stride (elements of T, sample_stride >= n_samples); out_elems must be batch * m * n_out else
 * SGX_DIM_MISMATCH; mem_kind as sgx_execute, `stream` a hipStream_t as its hip_stream.
 * Not offered (SGX_INVALID_INPUT, the text names the field): dither != 0, vtln_warp != 1, spectrogram != 0 (kaldi.spectrogram, a plan
 * without a bank), min_duration != 0, streaming != 0 (push / flush; the features are frame-local, so they can move onto the streaming
 * stage later).  Other errors (SGX_INVALID_INPUT), after torchaudio's asserts: N < 2, shift < 1, P > 2^20, low_freq outside
 * [0, fs / 2), high_freq outside (0, fs / 2], low_freq >= high_freq, preemphasis_coefficient outside [0, 1], num_ceps > num_mel_bins,
 * num_mel_bins <= 3 (or above 8192), an unknown window_type, dtype or route.  device -1: the current device, -2: a host-only plan (every
 * accessor below; execute and reserve return SGX_BACKEND behind their shape checks). */
typedef struct sgx_kaldi sgx_kaldi; /* opaque; same single-caller rule as sgx_fir */
enum { SGX_KALDI_WIN_HANNING = 0, SGX_KALDI_WIN_HAMMING = 1, SGX_KALDI_WIN_POVEY = 2, SGX_KALDI_WIN_RECTANGULAR = 3, SGX_KALDI_WIN_BLACKMAN = 4 };
enum { SGX_KALDI_ROUTE_AUTO = 0, SGX_KALDI_ROUTE_GENERIC = 1 };
typedef struct sgx_kaldi_params {
    double sample_frequency, frame_length_ms, frame_shift_ms;
    double blackman_coeff, preemphasis_coefficient, energy_floor, low_freq, high_freq;
    double dither, vtln_warp, min_duration, cepstral_lifter;
    int32_t window_type, remove_dc_offset, raw_energy, round_to_power_of_two, snip_edges;
    int32_t use_energy, use_power, use_log_fbank, htk_compat, subtract_mean;
    int32_t spectrogram, streaming; /* must be 0 */
    uint32_t num_mel_bins, num_ceps; /* num_ceps 0: fbank */
    int32_t dtype, device;
} sgx_kaldi_params;
sgx_status sgx_kaldi_create(const sgx_kaldi_params *params, int32_t route, size_t max_scratch_bytes, sgx_kaldi **out);
void sgx_kaldi_destroy(sgx_kaldi *plan);
size_t sgx_kaldi_window_size(const sgx_kaldi *plan);        /* N */
size_t sgx_kaldi_window_shift(const sgx_kaldi *plan);       /* shift */
size_t sgx_kaldi_padded_window_size(const sgx_kaldi *plan); /* P */
size_t sgx_kaldi_n_out(const sgx_kaldi *plan);              /* features per frame */
size_t sgx_kaldi_n_frames(const sgx_kaldi *plan, size_t n_samples); /* m; 0 when n_samples < N */
sgx_status sgx_kaldi_window(const sgx_kaldi *plan, double *window /* [N] */);
sgx_status sgx_kaldi_mel_banks(const sgx_kaldi *plan, double *banks /* dense [num_mel_bins][P / 2 + 1] */);
sgx_status sgx_kaldi_dct(const sgx_kaldi *plan, double *dct /* [num_ceps][num_mel_bins] */);
sgx_status sgx_kaldi_lifter(const sgx_kaldi *plan, double *lifter /* [num_ceps] */);
sgx_status sgx_kaldi_execute(sgx_kaldi *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                             int32_t mem_kind, void *stream);
/* Pre-sizes the generic route's chunk scratch and the internal plan's and, with host_staging, the SGX_MEM_HOST staging for calls of up
 * to `batch` rows of n_samples samples, so that those calls do not allocate. */
sgx_status sgx_kaldi_reserve(sgx_kaldi *plan, size_t batch, size_t n_samples, int32_t host_staging);
/* A diagnostic: how many times the plan has allocated or replaced one of its own buffers. */
size_t sgx_kaldi_allocations(const sgx_kaldi *plan);
size_t sgx_kaldi_tile(const sgx_kaldi *plan);             /* frames per workgroup tile of "k_kaldi"; 0 on the generic route */
const char *sgx_kaldi_kernel_name(const sgx_kaldi *plan); /* "k_kaldi" or "kaldi_generic" */
int32_t sgx_kaldi_device(const sgx_kaldi *plan);
const char *sgx_kaldi_last_error(const sgx_kaldi *plan); /* NULL plan: the text of the last failed create */

#ifdef __cplusplus
}
#endif
#endif /* SPECTRO_HIP_H */

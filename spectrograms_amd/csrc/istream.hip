// istream.hip — streaming inverse STFT plans (sgx_istream_*) of libspectro_hip.so: frames that arrive in runs, samples out as soon
// as no later frame can change them, the unfinished overlap tail carried on the device; kernel and host side.
//
// Reference: istft (src/spectrogram.rs:4860-4946) wants every frame of a signal at once; python/examples/streaming.py is the use
// case.  A stream here is the inverse of stream.hip's: `batch` rows in lock step, any number of new frames per call.
//
// Semantics.  Let pad = centre ? n_fft / 2 : 0; positions are those of the untrimmed signal; F counts the frames taken since
// creation, reset or flush; E(F) = (F - 1) hop + n_fft is the end of frame F - 1.
//   hi(F) = max(pad, min(F hop, E(F) - pad)), hi(0) = pad: positions below it are final (no later frame reaches below F hop, and the
//       last pad samples are the centre trim's if the stream ends here).
//   push(f >= 1 frames per row)   returns positions [hi(F), hi(F + f)): possibly none (out may be NULL, out_elems 0).
//   flush                         returns [hi(F), E(F) - pad); the one exception is the reference's quirk (:4933-4941): centre, even
//       n_fft and exactly one frame in total give the whole untrimmed frame [0, n_fft) (such a stream has emitted nothing yet).  A
//       stream that has taken no frame emits nothing.  The stream then stands as after reset, except that its row count stays fixed.
//   The first push after creation or reset fixes the row count; a later push with another one is SGX_DIM_MISMATCH.
// After the flush the samples of all calls, laid end to end, are those of sgx_istft on all frames at once: sgx_istft_length(F)
// samples in the same order, equal to rounding.  Not bit for bit: the rows' launcher may choose by row count, the paired routes
// pair the frames of a call, and the offline plan may take a fused kernel.
// The carry holds positions [c(F), E(F)) of every row as raw partial sums, c(F) = hi(F) (0 while the quirk can still apply: F = 1,
// centre, even n_fft): at most n_fft samples per row.  A sample whose frames arrive in two calls is therefore the same chain of
// additions as k_istft_ola's: the windowed row values of the covering frames in ascending frame order from T(0), then one division
// by norm = the sum of the rounded w w over ALL covering frames by absolute frame index, recomputed from the window (never
// carried), where norm > T(1e-10).  The imaginary parts of the DC bin (and of the Nyquist bin at even n_fft) are ignored as on the
// device path of sgx_istft and not reported: a stream does not synchronise to read a flag.
//
// Device side.  A call is two launches on the caller's stream:
//   launch_c2r_frames   (plan.hip, the rows of sgx_istft's unfused route) of a sibling sgx_plan that owns the window and the inverse
//                       tables: the f new frames, read with the caller's bin stride, windowed, into the frame scratch [rows][f][n_fft];
//   k_istream_ola<T>    one work item per position of [p0, E(F + f)), p0 = c(F): carry_prev, plus the new frames that cover it;
//                       positions in [hi(F), hi(F + f)) are normalised and stored to `out`, those from c(F + f) on go raw into
//                       carry_next.  The two carry buffers alternate, so no launch reads what it writes.  A flush is the same kernel
//                       with no new frame.
// k_istream_ola moves at most (n_fft + f hop) samples per row against the rows' f (n_fft / 2 + 1) complex bins in and f n_fft reals
// out, and reads n_fft / hop values per sample from a scratch that the rows have just written (L2 / Infinity Cache): it is small
// beside the rows and is left in the plainest shape that meets the store rules — no LDS, no cross-lane work, consecutive lanes on
// consecutive positions of one row so that a wave stores 256 (f64: 512) contiguous bytes per instruction, one element per lane
// (a row of `out` starts at any element, so wider stores would need an alignment prologue per row), up to 2048 workgroups that
// stride over what is beyond them.  Nothing here was tuned blind; tools/time_streaming_inverse.py times whole pushes.
// Buffer growth follows stream.hip: only the carry buffer NOT holding the carry and the frame scratch are ever replaced inside a
// call; their last readers were enqueued by the calls before, so the call's stream is synchronised in front of the release (and
// hipFree waits for the device).  A call within what sgx_istream_reserve sized allocates nothing and does not synchronise.
#include <algorithm>
#include <new>
#include <string>

#include "plan_host.h"

using namespace sgx;

namespace {

typedef unsigned long long u64;

struct IolaArgs {
    const void *frames;      // [rows][f][n] windowed rows of the call's new frames (f == 0: not read)
    const void *win;         // [n]
    const void *carry_prev;  // [rows][n]: positions [c0, c0 + clen) (clen == 0: not read)
    void *carry_next;        // [rows][n]: positions [c1, ..)
    void *out;               // [rows][e1 - e0]: positions [e0, e1)
    u64 p0, span;            // a row's work items: positions [p0, p0 + span)
    u64 c0, clen, c1, e0, e1;
    u64 F, f;                // frames before the call, new frames
    u64 total;               // rows * span
    unsigned n, hop;
};

template <typename T>
__global__ __launch_bounds__(256) void k_istream_ola(IolaArgs a) {
    const T *win = (const T *)a.win;
    const u64 n = a.n, hop = a.hop, last = a.F + a.f - 1, m = a.e1 - a.e0;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < a.total; i += (u64)gridDim.x * 256u) {
        const u64 r = i / a.span, pos = a.p0 + i % a.span;
        const u64 f_hi = min(pos / hop, last);
        const u64 f_lo = pos >= n ? (pos - n) / hop + 1 : 0;
        T acc = T(0);
        if (pos >= a.c0 && pos - a.c0 < a.clen) acc = ((const T *)a.carry_prev)[r * n + (pos - a.c0)];
        const T *fr = (const T *)a.frames + r * a.f * n;
        for (u64 g = max(f_lo, a.F); g <= f_hi; ++g) acc += fr[(g - a.F) * n + (pos - g * hop)];
        if (pos >= a.c1) ((T *)a.carry_next)[r * n + (pos - a.c1)] = acc;
        if (pos >= a.e0 && pos < a.e1) {
            // (the product is rounded before it is added: __fmul_rn / __fadd_rn are plain operators in the HIP headers, which hipcc's
            // default contraction would fuse into one fma)
            T nrm = T(0);
            for (u64 g = f_lo; g <= f_hi; ++g) {
#pragma clang fp contract(off)
                const T w = win[pos - g * hop];
                const T ww = w * w;
                nrm = nrm + ww;
            }
            if (nrm > T(1e-10)) acc /= nrm;
            ((T *)a.out)[r * m + (pos - a.e0)] = acc;
        }
    }
}

unsigned grid_for(u64 total) {  // 2048 workgroups (8 per CU) walk what is beyond them
    const u64 g = (total + 255) / 256;
    return (unsigned)std::max<u64>(1, std::min<u64>(g, 2048));
}

}  // namespace

struct sgx_istream {
    size_t n_fft = 0, hop = 0, pad = 0, n_bins = 0;
    bool whole = false;  // centre and even n_fft: one frame in total comes back untrimmed (the reference's quirk)
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    PlanHandle sib;    // the window and the inverse tables (the caller's parameters)
    DevBuf carry[2];   // [rows][n_fft] T each
    DevBuf frames;     // [rows][f][n_fft] T: the windowed rows of a call
    int cur = 0;       // the buffer that holds the carry (when F > 0)
    size_t F = 0, emitted = 0;  // frames taken and samples returned per row since creation / reset / flush
    size_t rows = 0;            // fixed by the first push after creation / reset (0: not fixed); flush keeps it
    size_t allocations = 0;     // (re)allocations of the stream's own buffers
    std::string route;          // sgx_istream_kernel_name
    DevBuf d_in, d_out;         // staging of the SGX_MEM_HOST calls
    mutable std::string err;
};

namespace {

size_t extent(const sgx_istream *s, size_t F) { return F ? (F - 1) * s->hop + s->n_fft : 0; }
size_t hi(const sgx_istream *s, size_t F) {
    return F ? std::max(s->pad, std::min(F * s->hop, extent(s, F) - s->pad)) : s->pad;
}
bool quirk(const sgx_istream *s, size_t F) { return s->whole && F == 1; }
size_t carry_start(const sgx_istream *s, size_t F) { return quirk(s, F) ? 0 : hi(s, F); }
size_t pending(const sgx_istream *s, size_t F) { return F ? extent(s, F) - carry_start(s, F) : 0; }
// the positions a flush after F frames returns
void flush_range(const sgx_istream *s, size_t F, size_t *e0, size_t *e1) {
    if (F == 0) { *e0 = *e1 = s->pad; }
    else if (quirk(s, F)) { *e0 = 0; *e1 = s->n_fft; }
    else { *e0 = hi(s, F); *e1 = extent(s, F) - s->pad; }
}

sgx_status grow_counted(sgx_istream *s, DevBuf &b, size_t need, hipStream_t hs, bool in_call) {
    if (b.bytes >= need) return SGX_OK;
    if (in_call && b.ptr) SGX_TRY_HIP(s, hipStreamSynchronize(hs));  // its last readers (the header comment)
    ++s->allocations;
    return grow(s, b, need);
}

// the sibling's global-memory scratch for `rows` x `f` frames, where its rows go that way (launch_c2r_frames grows it otherwise)
sgx_status big_reserve(sgx_istream *s, size_t rows, size_t f) {
    sgx_plan *pl = s->sib.get();
    if (pl->kind != K_BIGFFT && !pl->big.M) return SGX_OK;
    if (grow(pl, pl->d_big, big_scratch_bytes(pl->big, pl->dtype, rows * ((f + 1) / 2))) != SGX_OK) return fail(s, SGX_BACKEND, sgx_last_error(pl));
    return SGX_OK;
}

// one call on device pointers: f new frames (f == 0: a flush) onto the carry of F frames; positions [e0, e1) to `out`, the carry of
// F + f frames (a push) to the other buffer
sgx_status run_dev(sgx_istream *s, const void *spec, size_t rows, size_t f, size_t bin_stride, size_t e0, size_t e1, void *out,
                   hipStream_t hs, std::string *route) {
    sgx_plan *pl = s->sib.get();
    const size_t n = s->n_fft, F = s->F;
    const int nxt = s->cur ^ 1;
    sgx_status st;
    if (f) {
        if ((st = grow_counted(s, s->carry[nxt], rows * n * s->elem, hs, true)) != SGX_OK) return st;
        if ((st = grow_counted(s, s->frames, rows * f * n * s->elem, hs, true)) != SGX_OK) return st;
        const char *r = "";
        if (launch_c2r_frames(pl, spec, s->frames, rows, f, bin_stride, true, pl->d_window, hs, &r) != SGX_OK)
            return fail(s, SGX_BACKEND, sgx_last_error(pl));
        route->assign(r).append("+stream_ola");
    }
    IolaArgs a{};
    a.frames = s->frames; a.win = pl->d_window;
    a.carry_prev = F ? s->carry[s->cur].ptr : nullptr;
    a.c0 = carry_start(s, F); a.clen = pending(s, F);
    a.carry_next = s->carry[nxt];
    a.c1 = f ? carry_start(s, F + f) : extent(s, F);  // a flush carries nothing on
    a.out = out; a.e0 = e0; a.e1 = e1;
    a.p0 = F ? a.c0 : std::min<u64>(a.c1, s->pad);
    a.span = extent(s, F + f) - a.p0;
    a.F = F; a.f = f; a.n = unsigned(n); a.hop = unsigned(s->hop);
    a.total = u64(rows) * a.span;
    if (a.total == 0) return SGX_OK;
    if (s->dtype == SGX_F64) hipLaunchKernelGGL(k_istream_ola<double>, dim3(grid_for(a.total)), dim3(256), 0, hs, a);
    else hipLaunchKernelGGL(k_istream_ola<float>, dim3(grid_for(a.total)), dim3(256), 0, hs, a);
    SGX_TRY_HIP(s, hipGetLastError());
    return SGX_OK;
}

// push (f >= 1) and flush (f == 0, F >= 1) behind their argument checks; moves the state only when everything went out
sgx_status istream_call(sgx_istream *s, const void *spec, size_t rows, size_t f, size_t bin_stride, size_t e0, size_t e1, void *out,
                        size_t out_elems, int32_t mem_kind, void *stream) {
    const size_t m = e1 - e0, expect = rows * m;
    if (out_elems != expect) return dim_mismatch(s, expect, out_elems);
    if (m && !out) return fail(s, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (rows > 65535 || f > 0x7fffffffull || s->F + f > (size_t(1) << 40))
        return fail(s, SGX_INVALID_INPUT, "Invalid input: batch or frame count too large");
    if (s->device == -2) return fail(s, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(s, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    if (mem_kind == SGX_MEM_HOST && bin_stride != f) return fail(s, SGX_INVALID_INPUT, "Invalid input: SGX_MEM_HOST needs bin_stride == n_frames");
    hipStream_t hs = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(s, dg.enter(s->device));
    sgx_status st;
    std::string route = s->route;
    if (mem_kind == SGX_MEM_DEVICE) {
        if ((st = run_dev(s, spec, rows, f, bin_stride, e0, e1, out, hs, &route)) != SGX_OK) return st;
    } else {
        const size_t in_bytes = rows * s->n_bins * f * 2 * s->elem, out_bytes = out_elems * s->elem;
        if ((st = grow_counted(s, s->d_in, in_bytes, hs, true)) != SGX_OK) return st;
        if ((st = grow_counted(s, s->d_out, out_bytes, hs, true)) != SGX_OK) return st;
        if (in_bytes) SGX_TRY_HIP(s, hipMemcpyAsync(s->d_in, spec, in_bytes, hipMemcpyHostToDevice, hs));
        if ((st = run_dev(s, s->d_in, rows, f, bin_stride, e0, e1, s->d_out, hs, &route)) != SGX_OK) return st;
        if (out_bytes) SGX_TRY_HIP(s, hipMemcpyAsync(out, s->d_out, out_bytes, hipMemcpyDeviceToHost, hs));
        SGX_TRY_HIP(s, hipStreamSynchronize(hs));
    }
    s->route.swap(route);
    if (f) s->cur ^= 1;
    s->F += f;
    s->emitted += m;
    s->rows = rows;
    return SGX_OK;
}

void restart(sgx_istream *s) { s->F = s->emitted = 0; }

}  // namespace

extern "C" {

sgx_status sgx_istream_create(const sgx_params *params, sgx_istream **out) {
    if (out) *out = nullptr;
    if (!params || !out) return fail<sgx_istream>(nullptr, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (params->freq_scale == SGX_FREQ_CQT)
        return fail<sgx_istream>(nullptr, SGX_INVALID_INPUT, "Invalid input: an inverse stream inverts STFT frames (a CQT plan has no FFT)");
    sgx_istream *s = new (std::nothrow) sgx_istream();
    if (!s) return fail<sgx_istream>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    sgx_plan *raw = nullptr;
    const sgx_status st = sgx_plan_create(params, &raw);  // every check of the offline plan
    s->sib.reset(raw);
    if (st != SGX_OK) {
        delete s;
        return fail<sgx_istream>(nullptr, st, sgx_last_create_error());
    }
    s->n_fft = params->n_fft; s->hop = params->hop_size;
    s->pad = params->centre ? params->n_fft / 2 : 0;
    s->whole = params->centre && params->n_fft % 2 == 0;
    s->n_bins = params->n_fft / 2 + 1;
    s->dtype = params->dtype; s->elem = elem_size(params->dtype);
    s->device = sgx_plan_device(raw);
    *out = s;
    return SGX_OK;
}

void sgx_istream_destroy(sgx_istream *s) {
    if (!s) return;
    DeviceGuard dg;
    if (s->device != -2) (void)dg.enter(s->device);
    delete s;
}

sgx_status sgx_istream_step(const sgx_istream *s, size_t frames_taken, size_t n_frames, size_t *n_samples) {
    if (!s || !n_samples) return fail(s, SGX_INVALID_INPUT, "Invalid input: null argument");
    size_t e0 = 0, e1 = 0;
    if (n_frames) { e0 = hi(s, frames_taken); e1 = hi(s, frames_taken + n_frames); }
    else flush_range(s, frames_taken, &e0, &e1);
    *n_samples = e1 - e0;
    return SGX_OK;
}

size_t sgx_istream_frames_taken(const sgx_istream *s) { return s ? s->F : 0; }
size_t sgx_istream_samples_emitted(const sgx_istream *s) { return s ? s->emitted : 0; }
size_t sgx_istream_pending(const sgx_istream *s) { return s ? pending(s, s->F) : 0; }
size_t sgx_istream_allocations(const sgx_istream *s) { return s ? s->allocations : 0; }

sgx_status sgx_istream_flush_samples(const sgx_istream *s, size_t *n_samples) {
    return sgx_istream_step(s, s ? s->F : 0, 0, n_samples);
}

sgx_status sgx_istream_push(sgx_istream *s, const void *spec, size_t batch, size_t n_bins, size_t n_frames, size_t bin_stride, void *out,
                            size_t out_elems, int32_t mem_kind, void *stream) {
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (batch == 0 || n_frames == 0) return fail(s, SGX_INVALID_INPUT, "Invalid input: stft matrix must be non-empty");
    if (!spec) return fail(s, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (n_bins != s->n_bins) return dim_mismatch(s, s->n_bins, n_bins);
    if (bin_stride < n_frames) return fail(s, SGX_INVALID_INPUT, "Invalid input: bin_stride < n_frames");
    if (s->rows && batch != s->rows) return dim_mismatch(s, s->rows, batch, " (rows of the stream; reset() releases them)");
    return istream_call(s, spec, batch, n_frames, bin_stride, hi(s, s->F), hi(s, s->F + n_frames), out, out_elems, mem_kind, stream);
}

sgx_status sgx_istream_flush(sgx_istream *s, void *out, size_t out_elems, int32_t mem_kind, void *stream) {
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (s->F == 0) {  // nothing carried: no launch
        if (out_elems != 0) return dim_mismatch(s, 0, out_elems);
    } else {
        size_t e0 = 0, e1 = 0;
        flush_range(s, s->F, &e0, &e1);
        const sgx_status st = istream_call(s, nullptr, s->rows, 0, 0, e0, e1, out, out_elems, mem_kind, stream);
        if (st != SGX_OK) return st;
    }
    restart(s);
    return SGX_OK;
}

sgx_status sgx_istream_reset(sgx_istream *s, void *stream) {
    (void)stream;  // a dropped carry is never read again: nothing to enqueue
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    restart(s);
    s->rows = 0;
    return SGX_OK;
}

sgx_status sgx_istream_reserve(sgx_istream *s, size_t batch, size_t max_frames, int32_t host_staging) {
    if (!s || batch == 0 || max_frames == 0) return fail(s, SGX_INVALID_INPUT, "Invalid input: stft matrix must be non-empty");
    if (s->device == -2) return fail(s, SGX_BACKEND, kNoDeviceText);
    if (s->rows && batch > s->rows) return dim_mismatch(s, s->rows, batch, " (rows of the stream; reset() releases them)");
    if (s->F)
        return fail(s, SGX_INVALID_INPUT, "Invalid input: reserve() needs a stream without carried samples (after creation, reset or flush)");
    DeviceGuard dg;
    SGX_TRY_HIP(s, dg.enter(s->device));
    SGX_TRY_HIP(s, hipDeviceSynchronize());
    sgx_status st;
    const size_t row_bytes = s->n_fft * s->elem;
    for (int i = 0; i < 2; ++i)
        if ((st = grow_counted(s, s->carry[i], batch * row_bytes, nullptr, false)) != SGX_OK) return st;
    if ((st = grow_counted(s, s->frames, batch * max_frames * row_bytes, nullptr, false)) != SGX_OK) return st;
    if ((st = big_reserve(s, batch, max_frames)) != SGX_OK) return st;
    if (host_staging) {  // a push of f frames returns at most f hop + n_fft samples per row, a flush at most n_fft
        if ((st = grow_counted(s, s->d_in, batch * s->n_bins * max_frames * 2 * s->elem, nullptr, false)) != SGX_OK) return st;
        if ((st = grow_counted(s, s->d_out, batch * (max_frames * s->hop + s->n_fft) * s->elem, nullptr, false)) != SGX_OK) return st;
    }
    return SGX_OK;
}

const char *sgx_istream_kernel_name(const sgx_istream *s) { return s ? s->route.c_str() : ""; }
int32_t sgx_istream_device(const sgx_istream *s) { return s ? s->device : -2; }
const char *sgx_istream_last_error(const sgx_istream *s) { return s ? s->err.c_str() : create_err<sgx_istream>().c_str(); }

}  // extern "C"

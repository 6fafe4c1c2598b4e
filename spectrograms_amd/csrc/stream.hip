// stream.hip — streaming spectrogram plans (sgx_stream_*) of libspectro_hip.so: signals that arrive in blocks, the rows' pending
// samples carried on the device, kernel and host side.
//
// Reference: SpectrogramPlan::compute_frame (src/spectrogram.rs:335-372, python/examples/streaming.py) computes one column from the
// span it covers; a stream here is the batched form of that loop: `batch` rows in lock step, any block length per call.
//
// Semantics.  Let pad = centre ? n_fft / 2 : 0.  The stream holds a pending run of p virtual samples per row (the same p for every
// row: host state).  After creation or reset p = pad (zeros) and frames_emitted = 0.
//   push(C >= 1 samples per row):  P = p + C;  f = P >= n_fft ? (P - n_fft) / hop + 1 : 0;  the frames start at pending offsets
//       0, hop, .., (f - 1) hop;  afterwards p = P - f hop  (hop <= n_fft, so 0 <= p, and p < n_fft).  A call with f = 0 is legal: it
//       stages the block only, leaves `out` untouched and wants out_elems = 0.
//   flush:  appends pad zeros and emits the frames that then fit.  A stream that has taken samples but emitted no frame since its
//       reset (centre = 0, fewer than n_fft samples in total) emits the reference's single zero-filled frame (frame_count,
//       :1239-1242).  A stream that has taken no sample since its reset emits nothing.  The stream then stands as after reset,
//       except that its row count stays fixed.
//   The first push after creation or reset fixes the row count; a later push with another one is SGX_DIM_MISMATCH.
// After flush the frames of all calls, laid end to end, are the frames of the offline plan (sgx_execute, the same sgx_params) on
// the whole signals: the same count in the same order.  Equal to rounding, not bit for bit: the frame count of a call decides the
// launch shape, and a call of few frames may step down the plan's kernel chain (sgx_kernel_name), so another cut of the same signal
// can run another variant of the transform.  What IS exact is the staging: a push returns the bits of the no-centre plan on the rows
// pending | block.
//
// Device side.  The frames go through the plan kernels unchanged: the stream owns a no-centre sibling sgx_plan (the same parameters,
// centre = 0) and two work buffers [rows][pitch] of T, pitch a multiple of 16 bytes.  A call is two launches:
//   k_stream_stage<T>   writes work_next[r][0, p) from work_prev[r][consumed, consumed + p) (consumed = the previous call's f hop;
//                       zeros after a reset) and work_next[r][p, P) from the caller's row x + r sample_stride (zeros for a flush),
//                       one work item per 16-byte vector of the destination;
//   sgx_execute         (device path) of the sibling on work_next with n_samples = P, sample_stride = pitch, into the caller's `out`.
// The buffers alternate, so no launch reads what it writes.  Each buffer has its own pitch; one that is too small for the call's P
// (or row count) is replaced before the stage launch, sized for the largest P this block length can meet, n_fft - 1 + C.  The
// buffer to be replaced is the one NOT holding the pending samples; its last readers are the stage kernel of the previous call and
// the transform of the call before that, all enqueued on the caller's stream(s).  The rule relied on is grow's (plan_host.h):
// hipFree waits for the device, so every launch that reads the old buffer has run before it is released; the call's stream is
// synchronised in front of it as well, so the rule does not rest on hipFree alone.  Such a call cannot be captured; a call within
// what sgx_stream_reserve sized allocates nothing and does not synchronise.
#include <algorithm>
#include <new>
#include <string>

#include "plan_host.h"

using namespace sgx;

namespace {

// One 16-byte vector of a destination row: columns [c0, c0 + VE) of  carry[0, p) | block[p, P) | zeros.  `carry` and `block` are
// the row's sources (null: zeros).  A vector that lies inside one source whose address there is 16-byte aligned is one vector load;
// the seam, the row's end and unaligned sources go element by element.
template <typename T>
__device__ __forceinline__ void stage_vector(const T *carry, const T *block, unsigned long long p, unsigned long long P, unsigned long long c0, T *dst) {
    constexpr unsigned VE = 16 / sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(VE)));
    const T *src = nullptr;
    if (c0 + VE <= p) src = carry ? carry + c0 : nullptr;
    else if (c0 >= p && c0 + VE <= P) src = block ? block + (c0 - p) : nullptr;
    Vec o;
    if (src && (reinterpret_cast<unsigned long long>(src) & 15ull) == 0) {
        o = *reinterpret_cast<const Vec *>(src);
    } else {
#pragma unroll
        for (unsigned j = 0; j < VE; ++j) {
            const unsigned long long c = c0 + j;
            T v = T(0);
            if (c < p) { if (carry) v = carry[c]; }
            else if (c < P) { if (block) v = block[c - p]; }
            o[j] = v;
        }
    }
    *reinterpret_cast<Vec *>(dst + c0) = o;
}

// work_next[r][0, nvec VE) for every row r: nvec = ceil(P / VE) vectors per row, nvec VE <= out_pitch; total = rows nvec
template <typename T>
__global__ __launch_bounds__(256) void k_stream_stage(const T *prev, unsigned long long in_pitch, unsigned long long consumed, unsigned long long p,
                                                      const T *x, unsigned long long sample_stride, unsigned long long P, T *next,
                                                      unsigned long long out_pitch, unsigned long long nvec, unsigned long long total) {
    constexpr unsigned VE = 16 / sizeof(T);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long r = i / nvec, v = i % nvec;
        stage_vector<T>(prev ? prev + r * in_pitch + consumed : nullptr, x ? x + r * sample_stride : nullptr, p, P, v * VE, next + r * out_pitch);
    }
}

unsigned grid_for(unsigned long long total) {  // 2048 workgroups (8 per CU) walk what is beyond them
    const unsigned long long g = (total + 255) / 256;
    return (unsigned)std::max(1ull, std::min(g, 2048ull));
}

}  // namespace

struct sgx_stream {
    size_t n_fft = 0, hop = 0, pad = 0, n_bins = 0, cplx = 1;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    PlanHandle sib;  // the same parameters with centre = 0
    DevBuf work[2];  // [rows][pitch] T each
    size_t pitch[2] = {0, 0};
    int cur = 0;              // the buffer that holds the pending samples (when !fresh)
    bool fresh = true;        // the pending samples are the zeros after creation / reset / flush: nothing to read
    size_t consumed = 0;      // where they start in a row of work[cur]
    size_t p = 0, emitted = 0, pushed = 0;  // pending samples, frames and samples since creation / reset
    size_t rows = 0;          // fixed by the first push after creation / reset (0: not fixed); flush keeps it
    size_t allocations = 0;   // (re)allocations of the stream's own buffers
    DevBuf d_in, d_out;       // staging of the SGX_MEM_HOST calls
    mutable std::string err;
};

namespace {

size_t frames_of(const sgx_stream *s, size_t P) { return P >= s->n_fft ? (P - s->n_fft) / s->hop + 1 : 0; }

// what a flush emits now, and the length P of the rows it transforms
size_t flush_frames(const sgx_stream *s, size_t *P_out) {
    const size_t P = s->p + s->pad;
    size_t f = s->pushed ? frames_of(s, P) : 0;
    if (f == 0 && s->pushed && s->emitted == 0) f = 1;  // fewer than n_fft samples in total: the plan's one zero-filled frame
    if (P_out) *P_out = P;
    return f;
}

size_t round_pitch(const sgx_stream *s, size_t n) {
    const size_t ve = 16 / s->elem;
    return (n + ve - 1) / ve * ve;
}

// a stream-owned buffer of at least `need` bytes; counts the allocations
sgx_status grow_counted(sgx_stream *s, DevBuf &b, size_t need) {
    if (b.bytes >= need) return SGX_OK;
    ++s->allocations;
    return grow(s, b, need);
}

// work[i] for `rows` rows of up to `len` samples
sgx_status work_reserve(sgx_stream *s, int i, size_t rows, size_t len, hipStream_t hs, bool in_call) {
    if (s->pitch[i] >= len && s->work[i].bytes >= rows * s->pitch[i] * s->elem) return SGX_OK;
    const size_t pitch = std::max(s->pitch[i], round_pitch(s, len));
    if (in_call && s->work[i].ptr) SGX_TRY_HIP(s, hipStreamSynchronize(hs));  // its last readers (the header comment)
    s->pitch[i] = 0;
    const sgx_status st = grow_counted(s, s->work[i], rows * pitch * s->elem);
    if (st == SGX_OK) s->pitch[i] = pitch;
    return st;
}

void restart(sgx_stream *s) {
    s->p = s->pad;
    s->emitted = s->pushed = 0;
    s->fresh = true;
    s->consumed = 0;
}

// one call on device pointers: stage `C` samples per row (x null: zeros) behind the pending ones, transform f frames of the rows of P
sgx_status run_dev(sgx_stream *s, const void *x, size_t rows, size_t C, size_t stride, size_t P, size_t f, void *out, size_t out_elems,
                   hipStream_t hs) {
    const int nxt = s->cur ^ 1;
    sgx_status st = work_reserve(s, nxt, rows, std::max(P, s->n_fft - 1 + C), hs, true);
    if (st != SGX_OK) return st;
    const size_t ve = 16 / s->elem, nvec = (P + ve - 1) / ve;
    const unsigned long long total = (unsigned long long)rows * nvec;
    const void *prev = s->fresh ? nullptr : s->work[s->cur].ptr;
    if (s->dtype == SGX_F64)
        hipLaunchKernelGGL(k_stream_stage<double>, dim3(grid_for(total)), dim3(256), 0, hs, (const double *)prev, s->pitch[s->cur], s->consumed, s->p,
                           (const double *)x, stride, P, s->work[nxt].as<double>(), s->pitch[nxt], nvec, total);
    else
        hipLaunchKernelGGL(k_stream_stage<float>, dim3(grid_for(total)), dim3(256), 0, hs, (const float *)prev, s->pitch[s->cur], s->consumed, s->p,
                           (const float *)x, stride, P, s->work[nxt].as<float>(), s->pitch[nxt], nvec, total);
    SGX_TRY_HIP(s, hipGetLastError());
    if (f && sgx_execute(s->sib.get(), s->work[nxt], rows, P, s->pitch[nxt], out, out_elems, SGX_MEM_DEVICE, hs) != SGX_OK)
        return fail(s, SGX_BACKEND, sgx_last_error(s->sib.get()));
    return SGX_OK;
}

// push (x, C >= 1) and flush (x null, C = pad) behind their argument checks
sgx_status stream_call(sgx_stream *s, const void *x, size_t rows, size_t C, size_t stride, size_t P, size_t f, void *out, size_t out_elems,
                       int32_t mem_kind, void *stream) {
    const size_t expect = rows * s->n_bins * f * s->cplx;
    if (out_elems != expect) return dim_mismatch(s, expect, out_elems);
    if (f && !out) return fail(s, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (rows > 0xffffffffull || P > (size_t(1) << 40)) return fail(s, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
    if (s->device == -2) return fail(s, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(s, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t hs = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(s, dg.enter(s->device));
    sgx_status st;
    if (mem_kind == SGX_MEM_DEVICE) {
        if ((st = run_dev(s, x, rows, C, stride, P, f, out, out_elems, hs)) != SGX_OK) return st;
    } else {
        const size_t in_bytes = x ? ((rows - 1) * stride + C) * s->elem : 0, out_bytes = out_elems * s->elem;
        if ((st = grow_counted(s, s->d_in, in_bytes)) != SGX_OK) return st;
        if ((st = grow_counted(s, s->d_out, out_bytes)) != SGX_OK) return st;
        if (x) SGX_TRY_HIP(s, hipMemcpyAsync(s->d_in, x, in_bytes, hipMemcpyHostToDevice, hs));
        if ((st = run_dev(s, x ? s->d_in.ptr : nullptr, rows, C, stride, P, f, s->d_out, out_elems, hs)) != SGX_OK) return st;
        if (out_bytes) SGX_TRY_HIP(s, hipMemcpyAsync(out, s->d_out, out_bytes, hipMemcpyDeviceToHost, hs));
        SGX_TRY_HIP(s, hipStreamSynchronize(hs));
    }
    s->cur ^= 1;
    s->fresh = false;
    s->consumed = f * s->hop;
    s->p = P - std::min(P, f * s->hop);
    s->emitted += f;
    s->pushed += C;
    s->rows = rows;
    return SGX_OK;
}

}  // namespace

extern "C" {

sgx_status sgx_stream_create(const sgx_params *params, sgx_stream **out) {
    if (out) *out = nullptr;
    if (!params || !out) return fail<sgx_stream>(nullptr, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (params->freq_scale == SGX_FREQ_CQT)
        return fail<sgx_stream>(nullptr, SGX_INVALID_INPUT, "Invalid input: a stream runs the plans of sgx_plan_create (CQT plans do not stream)");
    sgx_stream *s = new (std::nothrow) sgx_stream();
    if (!s) return fail<sgx_stream>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    sgx_params sp = *params;
    sp.centre = 0;
    sgx_plan *raw = nullptr;
    const sgx_status st = sgx_plan_create(&sp, &raw);  // every check of the offline plan
    s->sib.reset(raw);
    if (st != SGX_OK) {
        delete s;
        return fail<sgx_stream>(nullptr, st, sgx_last_create_error());
    }
    s->n_fft = params->n_fft; s->hop = params->hop_size;
    s->pad = params->centre ? params->n_fft / 2 : 0;
    s->dtype = params->dtype; s->elem = elem_size(params->dtype);
    s->cplx = params->amp_scale == SGX_AMP_COMPLEX ? 2 : 1;
    s->device = sgx_plan_device(raw);
    size_t nf = 0;
    (void)sgx_output_shape(raw, s->n_fft, &s->n_bins, &nf);
    restart(s);
    *out = s;
    return SGX_OK;
}

void sgx_stream_destroy(sgx_stream *s) {
    if (!s) return;
    DeviceGuard dg;
    if (s->device != -2) (void)dg.enter(s->device);
    delete s;
}

sgx_status sgx_stream_step(const sgx_stream *s, size_t pending, size_t n_samples, size_t *n_frames, size_t *pending_after) {
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    const size_t P = pending + n_samples, f = frames_of(s, P);
    if (n_frames) *n_frames = f;
    if (pending_after) *pending_after = P - f * s->hop;
    return SGX_OK;
}

size_t sgx_stream_pending(const sgx_stream *s) { return s ? s->p : 0; }
size_t sgx_stream_frames_emitted(const sgx_stream *s) { return s ? s->emitted : 0; }
size_t sgx_stream_n_bins(const sgx_stream *s) { return s ? s->n_bins : 0; }
size_t sgx_stream_allocations(const sgx_stream *s) { return s ? s->allocations : 0; }

sgx_status sgx_stream_flush_frames(const sgx_stream *s, size_t *n_frames) {
    if (!s || !n_frames) return fail(s, SGX_INVALID_INPUT, "Invalid input: null argument");
    *n_frames = flush_frames(s, nullptr);
    return SGX_OK;
}

sgx_status sgx_stream_push(sgx_stream *s, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                           int32_t mem_kind, void *stream) {
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (batch == 0 || n_samples == 0) return fail(s, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (!x) return fail(s, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (sample_stride < n_samples) return fail(s, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    if (s->rows && batch != s->rows) return dim_mismatch(s, s->rows, batch, " (rows of the stream; reset() releases them)");
    const size_t P = s->p + n_samples;
    return stream_call(s, x, batch, n_samples, sample_stride, P, frames_of(s, P), out, out_elems, mem_kind, stream);
}

sgx_status sgx_stream_flush(sgx_stream *s, void *out, size_t out_elems, int32_t mem_kind, void *stream) {
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    size_t P = 0;
    const size_t f = flush_frames(s, &P);
    if (f == 0) {  // nothing to transform, and what is pending is dropped: no launch
        if (out_elems != 0) return dim_mismatch(s, 0, out_elems);
    } else {
        const sgx_status st = stream_call(s, nullptr, s->rows, s->pad, 0, P, f, out, out_elems, mem_kind, stream);
        if (st != SGX_OK) return st;
    }
    restart(s);
    return SGX_OK;
}

sgx_status sgx_stream_reset(sgx_stream *s, void *stream) {
    (void)stream;  // the zeros after a reset are not read from memory: nothing to enqueue
    if (!s) return fail(s, SGX_INVALID_INPUT, "Invalid input: null plan");
    restart(s);
    s->rows = 0;
    return SGX_OK;
}

sgx_status sgx_stream_reserve(sgx_stream *s, size_t batch, size_t max_block, int32_t host_staging) {
    if (!s || batch == 0 || max_block == 0) return fail(s, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (s->device == -2) return fail(s, SGX_BACKEND, kNoDeviceText);
    if (s->rows && batch > s->rows) return dim_mismatch(s, s->rows, batch, " (rows of the stream; reset() releases them)");
    if (!s->fresh)
        return fail(s, SGX_INVALID_INPUT, "Invalid input: reserve() needs a stream without pending samples (after creation, reset or flush)");
    DeviceGuard dg;
    SGX_TRY_HIP(s, dg.enter(s->device));
    const size_t len = s->n_fft - 1 + std::max(max_block, s->pad);  // the longest rows a push of max_block samples, or a flush, transforms
    sgx_status st;
    SGX_TRY_HIP(s, hipDeviceSynchronize());
    for (int i = 0; i < 2; ++i)
        if ((st = work_reserve(s, i, batch, len, nullptr, false)) != SGX_OK) return st;
    if (sgx_reserve(s->sib.get(), batch, len, 0, 0) != SGX_OK) return fail(s, SGX_BACKEND, sgx_last_error(s->sib.get()));
    if (host_staging) {
        const size_t f = std::max<size_t>(1, frames_of(s, len));
        if ((st = grow_counted(s, s->d_in, batch * max_block * s->elem)) != SGX_OK) return st;
        if ((st = grow_counted(s, s->d_out, batch * s->n_bins * f * s->cplx * s->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

const char *sgx_stream_kernel_name(const sgx_stream *s) { return s ? sgx_kernel_name(s->sib.get()) : ""; }
int32_t sgx_stream_device(const sgx_stream *s) { return s ? s->device : -2; }
const char *sgx_stream_last_error(const sgx_stream *s) { return s ? s->err.c_str() : create_err<sgx_stream>().c_str(); }

}  // extern "C"

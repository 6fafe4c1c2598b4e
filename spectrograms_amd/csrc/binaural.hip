// binaural.hip — binaural ITD / IPD / ILD / ILR spectrogram plans of libspectro_hip.so (C ABI: sgx_binaural_* in include/spectro_hip.h).
//
// Reference: src/binaural.rs.  Every map is two complex STFTs of the same shape (StftPlan::compute, src/spectrogram.rs:1424-1458), one
// per channel, followed by an elementwise function of the two spectra over the band of bins [start_bin, stop_bin):
//   bw = sr / n_fft,  start_bin = round(start_freq / bw),  stop_bin = round(end_freq / bw)   (f64, half away from zero)
//   magphase (:106-160), in T:  mag_sq = fma(re, re, im im);  mag_sq == 0: mag 0, phase (1, 0);  else mag = sqrt(mag_sq),
//                               phase = (re / mag, im / mag) as products with 1 / mag,  angle = atan2(phase.im, phase.re)
//   ITD (:472-560)   pow(magL) + pow(magR) > 0 ? (np_mod(aL - aR + pi, 2 pi) - pi) / (2 pi T(bw) T(k)) : 0   (pow: pow_mag, :57-84)
//   IPD (:830-900)   wrapped ? np_mod(aL - aR + pi, 2 pi) - pi : aL - aR
//   ILD (:1187-1240) magL + magR > 0 && magL > 0 && magR > 0 ? T(-20) log10(magR / magL) : NaN
//   ILR (:1530-1600) same condition, r = magR / magL:  r < 1 ? 1 - r : -(1 - 1 / r);  else NaN
// with np_mod(x, m) = fmod(fmod(x, m) + m, m) (:86-88).  Output [batch][stop_bin - start_bin][n_frames] T, frames contiguous.
//
// Routes:
//   fused     f32 n_fft 1024 (the complex plan on the tuned kernel): k_r32x16<OUT_BINAURAL, KIND, ...> (kernels_r32x16.hip) — the two
//             halves of a workgroup transform the left and the right tile of the same 16 frames with the unchanged passes 1 and 2, write
//             their X[k] to their own exchange buffer, and after one barrier the workgroup evaluates the band and stores it; the spectra
//             never leave the CU.  Every hop the one-signal tiles take (hop 256, the staged form, the per-lane loads); short signals too
//             (the packed walk of the mono plans is not used).  Built out with -DSGX_BIN_NO_FUSED for A/B timing.
//   generic   every shape: the plan's complex STFT (an sgx_plan with SGX_AMP_COMPLEX, i.e. the engine's own complex dispatch) runs on
//             the left rows and then the right rows of a chunk of signals into plan scratch, and k_binaural_epi<T, KIND> reads the band
//             rows of both spectra and writes the map.  Chunks hold at most kChunkBytes of spectra per channel.
//   histogram k_binaural_hist<T>: one workgroup per (signal, block of frames); the counts are integers in LDS (exact), then powi and the
//             per-column normalisation in f64 (:323-370, 691-740, 1043-1090, 1385-1430).
// The kind functions (binaural_kind.h) are the only place the arithmetic of the table above is written.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "binaural_kind.h"
#include "plan_host.h"

using namespace sgx;
using namespace sgx::binaural;

namespace {

// generic route: complex spectra per channel and chunk.  Sized so that the two channels' scratch together (192 MiB) could stay in the
// 256 MiB Infinity Cache between the transforms and the epilogue — a design intent, not measured (no counter run, no chunk sweep)
constexpr size_t kChunkBytes = size_t(96) << 20;
constexpr unsigned kHistMaxBins = 32768;  // k_binaural_hist: one column of counts in LDS (128 KiB)
constexpr size_t kHistLdsBytes = size_t(kHistMaxBins) * 4u;

// (the kernels below round every product and sum on its own, as the reference does)
#pragma clang fp contract(off)

// ---- generic epilogue -------------------------------------------------------------------------------------------------------------
// spec: [2][cb][nb][n_frames] complex T (left spectra, then right); out: [cb][n_bins][n_frames] T.  Block x = 256 frames of one row,
// grid y walks the cb * n_bins rows.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void k_binaural_epi(const T *__restrict__ spec, T *__restrict__ out, unsigned cb, unsigned nb,
                                                      unsigned n_frames, unsigned start_bin, unsigned n_bins, KindConst<T> c) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= n_frames) return;
    const size_t rows = (size_t)cb * n_bins, chan = (size_t)cb * nb * n_frames * 2u;
    for (size_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const size_t b = row / n_bins, r = row - b * n_bins, k = start_bin + r;
        const size_t i = ((b * nb + k) * n_frames + f) * 2u;
        const T *L = spec + i, *R = spec + chan + i;
        out[row * n_frames + f] = binaural_value<T, KIND>(L[0], L[1], R[0], R[1], (unsigned)k, c);
    }
}

// ---- histograms -------------------------------------------------------------------------------------------------------------------
// f64 powi as compiler-rt's __powidf2 computes it (the lowering of Rust's f64::powi)
__device__ __forceinline__ double powi_f64(double a, int b) {
    const bool recip = b < 0;
    double r = 1.0;
    while (true) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0 / r : r;
}

// values [batch][n_rows][n_frames] T -> out [batch][num_bins][n_frames] f64.  Workgroup (frame block, signal): FB frames, counts
// cnt[bin][FB] in LDS.  A value counts if it is finite and inside [lo, hi]; bin = min(floor((v - lo) / width) as usize, num_bins - 1)
// with Rust's saturating cast (NaN and negatives to 0).
template <typename T>
__global__ __launch_bounds__(256) void k_binaural_hist(const T *__restrict__ vals, double *__restrict__ out, unsigned batch, unsigned n_rows,
                                                       unsigned n_frames, unsigned num_bins, unsigned fb, double lo, double hi, double width,
                                                       int exponent, int normalize) {
    extern __shared__ unsigned cnt[];
    __shared__ double colsum[64];
    const unsigned f0 = blockIdx.x * fb, nfb = min(fb, n_frames - f0);
    for (unsigned b = blockIdx.y; b < batch; b += gridDim.y) {
        for (unsigned i = threadIdx.x; i < num_bins * fb; i += 256u) cnt[i] = 0u;
        __syncthreads();
        const T *v = vals + (size_t)b * n_rows * n_frames + f0;
        for (unsigned i = threadIdx.x; i < n_rows * fb; i += 256u) {
            const unsigned r = i / fb, f = i - r * fb;
            if (f >= nfb) continue;
            const double x = (double)v[(size_t)r * n_frames + f];
            if (!isfinite(x) || x < lo || x > hi) continue;
            const double q = floor((x - lo) / width);
            unsigned long long bi;
            if (!(q > 0.0)) bi = 0;  // NaN, 0 and negatives (as usize saturates at 0)
            else if (q >= 18446744073709551615.0) bi = ~0ull;
            else bi = (unsigned long long)q;
            if (bi > num_bins - 1u) bi = num_bins - 1u;
            atomicAdd(&cnt[bi * fb + f], 1u);
        }
        __syncthreads();
        // per column: powi (exponent != 1), then the sum in ascending bin order
        if (threadIdx.x < nfb) {
            double s = 0.0;
            for (unsigned k = 0; k < num_bins; ++k) {
                double h = (double)cnt[k * fb + threadIdx.x];
                if (exponent != 1) h = powi_f64(h, exponent);
                s += h;
            }
            colsum[threadIdx.x] = s;
        }
        __syncthreads();
        double *o = out + (size_t)b * num_bins * n_frames + f0;
        for (unsigned i = threadIdx.x; i < num_bins * fb; i += 256u) {
            const unsigned k = i / fb, f = i - k * fb;
            if (f >= nfb) continue;
            double h = (double)cnt[i];
            if (exponent != 1) h = powi_f64(h, exponent);
            if (normalize && colsum[f] > 0.0) h /= colsum[f];
            o[(size_t)k * n_frames + f] = h;
        }
        __syncthreads();
    }
}

}  // namespace

struct sgx_binaural {
    PlanHandle stft;  // the complex STFT of both channels (SGX_AMP_COMPLEX); host-only when the binaural plan is
    sgx_binaural_params bp{};
    int dtype = SGX_F32;
    size_t elem = 4;
    int device = -2;
    double sr = 0.0, bw = 0.0;
    unsigned n_fft = 0, hop = 0, nb = 0;
    size_t start_bin = 0, stop_bin = 0;
    std::string route;
    bool fused = false;  // f32 n_fft 1024 on the tuned kernel: both channels in one launch (launch_r32x16_binaural)
    DevBuf d_spec, d_in, d_out;  // chunk spectra [2][cb][nb][nf] complex; SGX_MEM_HOST staging
    mutable std::string err;
};

namespace {

// the inner plan's failure, re-reported on the binaural plan
sgx_status from_stft(sgx_binaural *p, sgx_status st) {
    return fail(p, st, sgx_last_error(p->stft.get()) ? sgx_last_error(p->stft.get()) : "");
}

size_t chunk_rows(const sgx_binaural *p, size_t batch, size_t nf) {
    const size_t per = size_t(p->nb) * nf * 2u * p->elem;
    return std::max<size_t>(1, std::min(batch, kChunkBytes / std::max<size_t>(per, 1)));
}

template <typename T>
hipError_t launch_epi(const sgx_binaural *p, const void *spec, void *out, unsigned cb, unsigned nf, hipStream_t s) {
    KindConst<T> c;
    c.pi = T(3.14159265358979323846264338327950288);
    c.two_pi = T(2) * c.pi;
    c.bw = T(p->bw);
    c.power = p->bp.magphase_power;
    c.wrapped = p->bp.wrapped;
    const unsigned n_bins = unsigned(p->stop_bin - p->start_bin), sb = unsigned(p->start_bin);
    const size_t rows = size_t(cb) * n_bins;
    const dim3 grid((nf + 255u) / 256u, unsigned(std::min<size_t>(rows, 65535)));
    const T *sp = static_cast<const T *>(spec);
    T *o = static_cast<T *>(out);
    switch (p->bp.kind) {
        case SGX_BINAURAL_ITD: hipLaunchKernelGGL((k_binaural_epi<T, SGX_BINAURAL_ITD>), grid, dim3(256), 0, s, sp, o, cb, p->nb, nf, sb, n_bins, c); break;
        case SGX_BINAURAL_IPD: hipLaunchKernelGGL((k_binaural_epi<T, SGX_BINAURAL_IPD>), grid, dim3(256), 0, s, sp, o, cb, p->nb, nf, sb, n_bins, c); break;
        case SGX_BINAURAL_ILD: hipLaunchKernelGGL((k_binaural_epi<T, SGX_BINAURAL_ILD>), grid, dim3(256), 0, s, sp, o, cb, p->nb, nf, sb, n_bins, c); break;
        default: hipLaunchKernelGGL((k_binaural_epi<T, SGX_BINAURAL_ILR>), grid, dim3(256), 0, s, sp, o, cb, p->nb, nf, sb, n_bins, c); break;
    }
    return hipGetLastError();
}

// fused route: the tuned kernel's tables from the complex plan, one launch for the whole batch; false: the shape is not the kernel's
bool fused_args(const sgx_binaural *p, StftArgs &a, const void *left, const void *right, size_t batch, size_t n_samples, size_t stride,
                size_t nf, void *out) {
    const sgx_plan *pl = p->stft.get();
    std::memset(&a, 0, sizeof(a));
    a.x = left;
    a.x2 = right;
    a.out = out;
    a.sample_stride = stride;
    a.n_samples = n_samples;
    a.batch = unsigned(batch);
    a.n_fft = 1024;
    a.m = 512;
    a.log2m = 9;
    a.hop = p->hop;
    a.pad = pl->p.centre ? 512u : 0u;
    a.n_frames = unsigned(nf);
    a.nb_fft = 513;
    a.n_out = unsigned(p->stop_bin - p->start_bin);
    a.window = pl->d_window_half;  // (w[2n], w[2n+1]) / 2, as the complex plan launches it
    a.tw = pl->d_tw;
    a.tw1 = pl->d_tw1;
    a.tw2 = pl->d_tw2;
    a.out_mode = OUT_BINAURAL;
    a.amp = p->bp.kind;
    a.bin_start = unsigned(p->start_bin);
    a.bin_count = a.n_out;
    a.bin_power = p->bp.magphase_power;
    a.bin_wrapped = p->bp.wrapped;
    a.bin_bw = float(p->bw);
    if (!plan_geometry_r32x16_f32(a)) return false;
    a.tiles = (a.n_frames + a.ft - 1) / a.ft;
    return (unsigned long long)a.tiles * batch < 0x7ffffff0ull;
}

// device pointers, on the plan's device
sgx_status run_dev(sgx_binaural *p, const void *left, const void *right, size_t batch, size_t n_samples, size_t stride, size_t nf,
                   void *out, hipStream_t s) {
    if (p->fused) {
        StftArgs a;
        if (fused_args(p, a, left, right, batch, n_samples, stride, nf, out)) {
            SGX_TRY_HIP(p, launch_r32x16_binaural(a, s));
            return SGX_OK;
        }
    }
    const size_t cb = chunk_rows(p, batch, nf), spec_elems = cb * p->nb * nf * 2u;
    sgx_status st;
    if ((st = grow(p, p->d_spec, 2u * spec_elems * p->elem)) != SGX_OK) return st;
    const size_t n_bins = p->stop_bin - p->start_bin;
    for (size_t b0 = 0; b0 < batch; b0 += cb) {
        const size_t n = std::min(cb, batch - b0), elems = n * p->nb * nf * 2u;
        unsigned char *specL = p->d_spec.as<unsigned char>(), *specR = specL + n * p->nb * nf * 2u * p->elem;
        const size_t in_off = b0 * stride * p->elem;
        if ((st = sgx_execute(p->stft.get(), static_cast<const unsigned char *>(left) + in_off, n, n_samples, stride, specL, elems, SGX_MEM_DEVICE, s)) != SGX_OK)
            return from_stft(p, st);
        if ((st = sgx_execute(p->stft.get(), static_cast<const unsigned char *>(right) + in_off, n, n_samples, stride, specR, elems, SGX_MEM_DEVICE, s)) != SGX_OK)
            return from_stft(p, st);
        void *o = static_cast<unsigned char *>(out) + b0 * n_bins * nf * p->elem;
        SGX_TRY_HIP(p, p->dtype == SGX_F64 ? launch_epi<double>(p, specL, o, unsigned(n), unsigned(nf), s)
                                      : launch_epi<float>(p, specL, o, unsigned(n), unsigned(nf), s));
    }
    return SGX_OK;
}

sgx_status check_freqs(const sgx_params &sp, const sgx_binaural_params &bp, std::string &msg) {
    // ITDSpectrogramParams::new (:410-460) and its siblings, in their order
    const double a = bp.start_freq, e = bp.end_freq, sr = sp.sample_rate_hz;
    if (a <= 0.0 || e <= 0.0) { msg = "Invalid input: Start and end frequencies must be positive."; return SGX_INVALID_INPUT; }
    if (a >= e) { msg = "Invalid input: Start frequency must be less than end frequency."; return SGX_INVALID_INPUT; }
    if (e > sr / 2.0) { msg = "Invalid input: End frequency must be less than Nyquist frequency."; return SGX_INVALID_INPUT; }
    // NaN passes the three tests above in the reference, which then rounds it to bin 0: refused here
    if (!std::isfinite(a) || !std::isfinite(e)) { msg = "Invalid input: Start and end frequencies must be finite."; return SGX_INVALID_INPUT; }
    return SGX_OK;
}

}  // namespace

extern "C" {

sgx_status sgx_binaural_create(const sgx_params *stft, const sgx_binaural_params *bp, sgx_binaural **out) {
    if (out) *out = nullptr;
    if (!out || !stft || !bp) return fail<sgx_binaural>(nullptr, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (bp->kind < SGX_BINAURAL_ITD || bp->kind > SGX_BINAURAL_ILR)
        return fail<sgx_binaural>(nullptr, SGX_INVALID_INPUT, "Invalid input: unknown binaural kind " + std::to_string(bp->kind));
    // the STFT fields only: a linear complex plan of the same framing, window and type
    sgx_params sp = *stft;
    sp.freq_scale = SGX_FREQ_LINEAR;
    sp.amp_scale = SGX_AMP_COMPLEX;
    sp.has_log_params = 0;
    sp.n_mels = 0;
    sp.n_mfcc = 0;
    sgx_plan *raw = nullptr;
    sgx_status st = sgx_plan_create(&sp, &raw);
    PlanHandle inner(raw);  // destroyed with every refusal below
    if (st != SGX_OK) return fail<sgx_binaural>(nullptr, st, sgx_last_create_error() ? sgx_last_create_error() : "");
    std::string msg;
    if ((st = check_freqs(sp, *bp, msg)) != SGX_OK) return fail<sgx_binaural>(nullptr, st, msg);
    if (bp->magphase_power == 0)  // NonZeroUsize in the reference (the Python binding maps 0 to 1)
        return fail<sgx_binaural>(nullptr, SGX_INVALID_INPUT, "Invalid input: magphase_power must be >= 1");
    const double bw = sp.sample_rate_hz / double(sp.n_fft);
    const double sb = std::round(bp->start_freq / bw), eb = std::round(bp->end_freq / bw);  // (f / bw).round() as usize
    const size_t nb = sp.n_fft / 2u + 1u;
    if (!(eb > sb) || eb > double(nb))  // an empty band: the reference panics at NonEmptyVec::new (:550)
        return fail<sgx_binaural>(nullptr, SGX_INVALID_INPUT, "Invalid input: Frequency range should have at least one bin");
    sgx_binaural *p = new (std::nothrow) sgx_binaural();
    if (!p) return fail<sgx_binaural>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->bp = *bp;
    p->dtype = sp.dtype;
    p->elem = elem_size(sp.dtype);
    p->device = sgx_plan_device(inner.get());
    p->sr = sp.sample_rate_hz;
    p->bw = bw;
    p->n_fft = sp.n_fft;
    p->hop = sp.hop_size;
    p->nb = unsigned(nb);
    p->start_bin = size_t(sb);
    p->stop_bin = size_t(eb);
#ifdef SGX_BIN_NO_FUSED  // A/B builds only (tools/time_binaural.py --ab): every shape on the generic route
    p->fused = false;
#else
    p->fused = sp.dtype == SGX_F32 && sp.n_fft == 1024u && inner->kind == K_R32X16_F32;
#endif
    p->route = p->fused ? std::string("r32x16_binaural_f32") : std::string("binaural_epilogue/") + sgx_kernel_name(inner.get());
    p->stft = std::move(inner);
    *out = p;
    return SGX_OK;
}

void sgx_binaural_destroy(sgx_binaural *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    delete p;
}

sgx_status sgx_binaural_output_shape(const sgx_binaural *p, size_t n_samples, size_t *start_bin, size_t *n_bins, size_t *n_frames) {
    if (!p || !start_bin || !n_bins || !n_frames) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    size_t nb, nf;
    const sgx_status st = sgx_output_shape(p->stft.get(), n_samples, &nb, &nf);
    if (st != SGX_OK) return fail(p, st, sgx_last_error(p->stft.get()) ? sgx_last_error(p->stft.get()) : "");
    *start_bin = p->start_bin;
    *n_bins = p->stop_bin - p->start_bin;
    *n_frames = nf;
    return SGX_OK;
}

sgx_status sgx_binaural_axes(const sgx_binaural *p, size_t n_frames, double *freqs, double *times) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (freqs)  // bin as f64 * bin_width (:541-545)
        for (size_t k = p->start_bin; k < p->stop_bin; ++k) freqs[k - p->start_bin] = double(k) * p->bw;
    if (times)  // frame as f64 * hop_size / sample_rate (:548-553)
        for (size_t f = 0; f < n_frames; ++f) times[f] = double(f) * double(p->hop) / p->sr;
    return SGX_OK;
}

sgx_status sgx_binaural_execute(sgx_binaural *p, const void *left, const void *right, size_t batch, size_t n_samples, size_t sample_stride,
                                void *out, size_t out_elems, int32_t mem_kind, void *hip_stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!left || !right || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || n_samples == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (sample_stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    if (batch > 0xffffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch too large");
    size_t sb, n_bins, nf;
    sgx_status st = sgx_binaural_output_shape(p, n_samples, &sb, &n_bins, &nf);
    if (st != SGX_OK) return st;
    if (nf > 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: too many frames");
    const size_t expected = batch * n_bins * nf;
    if (out_elems != expected)
        return dim_mismatch(p, expected, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return run_dev(p, left, right, batch, n_samples, sample_stride, nf, out, s);
    // host pointers: plan-owned staging (both channels' rows, then the map), synchronous
    const size_t in_bytes = ((batch - 1) * sample_stride + n_samples) * p->elem, out_bytes = expected * p->elem;
    if ((st = grow(p, p->d_in, 2u * in_bytes)) != SGX_OK) return st;
    if ((st = grow(p, p->d_out, out_bytes)) != SGX_OK) return st;
    unsigned char *dl = p->d_in.as<unsigned char>(), *dr = dl + in_bytes;
    SGX_TRY_HIP(p, hipMemcpyAsync(dl, left, in_bytes, hipMemcpyHostToDevice, s));
    SGX_TRY_HIP(p, hipMemcpyAsync(dr, right, in_bytes, hipMemcpyHostToDevice, s));
    if ((st = run_dev(p, dl, dr, batch, n_samples, sample_stride, nf, p->d_out, s)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

sgx_status sgx_binaural_histogram(sgx_binaural *p, const void *values, size_t batch, size_t n_frames, size_t num_bins, double lo, double hi,
                                  int32_t exponent, int32_t normalize, double *out, size_t out_elems, int32_t mem_kind, void *hip_stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!values || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || n_frames == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: values must be non-empty");
    if (num_bins == 0 || num_bins > kHistMaxBins)
        return fail(p, SGX_INVALID_INPUT, "Invalid input: num_bins must be in 1.." + std::to_string(kHistMaxBins));
    if (batch > 0xffffffffull || n_frames > 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or frame count too large");
    const size_t n_rows = p->stop_bin - p->start_bin, expected = batch * num_bins * n_frames;
    if (out_elems != expected)
        return dim_mismatch(p, expected, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    const size_t in_bytes = batch * n_rows * n_frames * p->elem, out_bytes = expected * 8u;
    const void *vin = values;
    double *vout = out;
    sgx_status st;
    if (mem_kind == SGX_MEM_HOST) {
        if ((st = grow(p, p->d_in, in_bytes)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, out_bytes)) != SGX_OK) return st;
        SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, values, in_bytes, hipMemcpyHostToDevice, s));
        vin = p->d_in;
        vout = p->d_out.as<double>();
    }
    // frames per workgroup: up to 64, as many as one column block of counts in kHistLdsBytes allows
    const unsigned nbins = unsigned(num_bins);
    const unsigned fb = unsigned(std::max<size_t>(1, std::min<size_t>({64, n_frames, kHistLdsBytes / (4u * nbins)})));
    const unsigned lds = nbins * fb * 4u;
    const dim3 grid(unsigned((n_frames + fb - 1) / fb), unsigned(std::min<size_t>(batch, 65535)));
    const double width = (hi - lo) / double(num_bins);
    if (p->dtype == SGX_F64) {
        SGX_TRY_HIP(p, set_max_dynamic_lds((const void *)k_binaural_hist<double>, int(kHistLdsBytes)));
        hipLaunchKernelGGL(k_binaural_hist<double>, grid, dim3(256), lds, s, static_cast<const double *>(vin), vout, unsigned(batch),
                           unsigned(n_rows), unsigned(n_frames), nbins, fb, lo, hi, width, exponent, normalize);
    } else {
        SGX_TRY_HIP(p, set_max_dynamic_lds((const void *)k_binaural_hist<float>, int(kHistLdsBytes)));
        hipLaunchKernelGGL(k_binaural_hist<float>, grid, dim3(256), lds, s, static_cast<const float *>(vin), vout, unsigned(batch),
                           unsigned(n_rows), unsigned(n_frames), nbins, fb, lo, hi, width, exponent, normalize);
    }
    SGX_TRY_HIP(p, hipGetLastError());
    if (mem_kind == SGX_MEM_HOST) {
        SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
        SGX_TRY_HIP(p, hipStreamSynchronize(s));
    }
    return SGX_OK;
}

sgx_status sgx_binaural_reserve(sgx_binaural *p, size_t batch, size_t n_samples, int32_t host_staging) {
    if (!p || batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    size_t sb, n_bins, nf;
    sgx_status st = sgx_binaural_output_shape(p, n_samples, &sb, &n_bins, &nf);
    if (st != SGX_OK) return st;
    const size_t cb = chunk_rows(p, batch, nf);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (!p->fused) {  // (the fused route needs no scratch)
        if ((st = sgx_reserve(p->stft.get(), cb, n_samples, 0, 0)) != SGX_OK) return from_stft(p, st);
        if ((st = grow(p, p->d_spec, 2u * cb * p->nb * nf * 2u * p->elem)) != SGX_OK) return st;
    }
    if (host_staging) {
        if ((st = grow(p, p->d_in, 2u * batch * n_samples * p->elem)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, batch * n_bins * nf * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

const char *sgx_binaural_kernel_name(const sgx_binaural *p) { return p ? p->route.c_str() : ""; }

int32_t sgx_binaural_device(const sgx_binaural *p) { return p ? p->device : -2; }

const char *sgx_binaural_last_error(const sgx_binaural *p) { return p ? p->err.c_str() : create_err<sgx_binaural>().c_str(); }

}  // extern "C"

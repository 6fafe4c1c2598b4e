// gammatone.hip — batched time-domain gammatone IIR spectrogram plans of libspectro_hip.so (C ABI: sgx_gammatone_* in
// include/spectro_hip.h), kernel and host side.
//
// Reference: src/erb.rs:405-654 (make_iir_bank :456-497, iir_gain :426-453, iir4_rms :529-541, hann_window :545-549,
// gammatone_iir_spectrogram :603-654).  Every (signal, frame, band) is its own recurrence: four cascaded second-order sections in Direct
// Form II transposed, f64, started from zero state at the frame's first sample, and the root mean square of the fourth section's output.
// There is no transform in it; the cost is 16 dependent-chain f64 operations plus one for the energy per sample per (frame, band).
//
// k_gammatone_iir<T>: one kernel for every shape and both types.
//   * The (frame, band) pairs of a signal are flattened, q = frame * n_bands + band, and a workgroup of 256 lanes takes pairs
//     [256 w, 256 w + 256): no lane idles on a band count that does not divide 64 (only the signal's last workgroup is partial).
//   * The frames those pairs belong to (256 / n_bands when that divides, never more than 129) are kept in LDS as windowed f64 samples, `chunk`
//     samples of each frame at a time: a chunk is loaded (T, coalesced along the frame), converted, multiplied by the window and stored;
//     then every lane walks its frame's row.  All lanes of a frame read the same address in a step (a broadcast); the rows of two frames
//     are chunk + 2 doubles apart (chunk a multiple of the 256-byte bank row where LDS allows), so a wave that straddles frames reads
//     different banks.  Walking a frame in chunks is exact: the eight state values, the three values in flight between the sections and
//     the running sum stay in registers.
//   * The four sections run one sample apart (section k works on sample j - k + 1 in step j), so a step is four independent
//     three-operation chains and the energy update, not one chain of twelve; the first three steps feed the later sections exact zeros
//     (their state stays zero), and three more steps after the last sample drain them (section 1 then runs on zeros nobody reads).
//   * Epilogue in the same launch: T(sqrt(sum / N)), and with a dB floor the T-typed 10 log10 of the other kernels (hardware log2 in
//     f32, db_f64.h in f64) above eps, the host's 10 log10(eps) at or below it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "db_f64.h"
#include "plan_host.h"

using namespace sgx;

namespace {

constexpr double kPiG = 3.14159265358979323846264338327950288;
constexpr unsigned kGtLanes = 256;
constexpr size_t kGtLds = 32 * 1024;  // LDS per workgroup: five workgroups (five waves per SIMD) per CU
constexpr unsigned kGtMaxFilters = 65536;
constexpr int kCoef = SGX_GAMMATONE_COEFFS;

struct GtArgs {
    const void *x;       // [batch][sample_stride] T
    void *out;           // [batch][n_bands][n_frames] T
    const double *win;   // [frame] f64
    const double *coef;  // [n_bands][kCoef] f64
    unsigned long long sample_stride, pairs;  // pairs = n_frames * n_bands
    unsigned frame, hop, n_frames, n_bands;
    unsigned wgs;      // workgroups per signal
    unsigned chunk;    // samples of a frame in LDS at a time (even)
    unsigned rstride;  // doubles between the rows of two frames in LDS (chunk + 2)
    int db;
    double eps, floor_val;  // T values held in f64: eps = T(10^(db_floor / 10)), floor_val = T(10) log10(eps) in T
};

__device__ __forceinline__ float gt_db(float v) { return __builtin_log2f(v) * 3.01029995663981195f; }
__device__ __forceinline__ double gt_db(double v) { return db_f64(v); }

template <typename T>
__global__ __launch_bounds__(kGtLanes) void k_gammatone_iir(GtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double gt_buf[];  // [frames of the workgroup][rstride]
    const unsigned tid = threadIdx.x;
    const unsigned wg = blockIdx.x % a.wgs, b = blockIdx.x / a.wgs;
    const unsigned long long q0 = (unsigned long long)wg * kGtLanes, q = q0 + tid;
    const unsigned long long qlast = min(q0 + (kGtLanes - 1u), a.pairs - 1u);
    const unsigned f0 = unsigned(q0 / a.n_bands), nf = unsigned(qlast / a.n_bands) - f0 + 1u;
    const bool act = q < a.pairs;
    const unsigned f = act ? unsigned(q / a.n_bands) : f0, band = act ? unsigned(q % a.n_bands) : 0u;

    const double *c = a.coef + (size_t)band * kCoef;
    const double a01 = c[0], a11 = c[1], a02 = c[2], a12 = c[3], a03 = c[4], a13 = c[5], a04 = c[6], a14 = c[7];
    const double nb1 = -c[8], nb2 = -c[9];
    double z01 = 0.0, z11 = 0.0, z02 = 0.0, z12 = 0.0, z03 = 0.0, z13 = 0.0, z04 = 0.0, z14 = 0.0;
    double y1 = 0.0, y2 = 0.0, y3 = 0.0;  // section outputs of the previous step: the next section's input in this one
    double acc = 0.0;
    // one step: section 1 takes x, sections 2..4 the outputs of the step before; y = a0 x + z0, z0 = (a1 x + z1) - b1 y, z1 = -b2 y
    auto step = [&](double x) {
        const double u1 = fma(a01, x, z01), u2 = fma(a02, y1, z02), u3 = fma(a03, y2, z03), u4 = fma(a04, y3, z04);
        z01 = fma(nb1, u1, fma(a11, x, z11));
        z02 = fma(nb1, u2, fma(a12, y1, z12));
        z03 = fma(nb1, u3, fma(a13, y2, z13));
        z04 = fma(nb1, u4, fma(a14, y3, z14));
        z11 = nb2 * u1;
        z12 = nb2 * u2;
        z13 = nb2 * u3;
        z14 = nb2 * u4;
        acc = fma(u4, u4, acc);
        y1 = u1;
        y2 = u2;
        y3 = u3;
    };

    const T *xs = (const T *)a.x + (size_t)b * a.sample_stride + (size_t)f0 * a.hop;  // the workgroup's first frame
    const double *row = gt_buf + (size_t)(f - f0) * a.rstride;
    for (unsigned c0 = 0; c0 < a.frame; c0 += a.chunk) {
        const unsigned len = min(a.chunk, a.frame - c0);
        __syncthreads();  // the chunk before has been walked
        for (unsigned idx = tid; idx < nf * len; idx += kGtLanes) {
            const unsigned fi = idx / len, i = idx - fi * len;
            gt_buf[(size_t)fi * a.rstride + i] = (double)xs[(size_t)fi * a.hop + c0 + i] * a.win[c0 + i];
        }
        __syncthreads();
        if (act) {
#pragma unroll 4
            for (unsigned i = 0; i < len; ++i) step(row[i]);
        }
    }
    if (!act) return;
    step(0.0);
    step(0.0);
    step(0.0);
    T v = T(sqrt(acc / double(a.frame)));
    if (a.db) v = v > T(a.eps) ? gt_db(v) : T(a.floor_val);
    ((T *)a.out)[((size_t)b * a.n_bands + band) * a.n_frames + f] = v;
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_gammatone {
    double sample_rate = 0.0;
    size_t frame = 0, hop = 0, n_bands = 0;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    bool db = false;
    double eps = 0.0, floor_val = 0.0;
    std::vector<double> centres, coef, window;  // coef [n_bands][kCoef]
    DevBuf d_win, d_coef, d_in, d_out;
    mutable std::string err;
};

namespace {

// iir_gain (src/erb.rs:426-453) from the centre frequency: complex values as (re, im) pairs with num_complex's formulas (product,
// powi(4) by squaring, quotient by the squared norm, hypot).  Evaluated in long double and rounded once: for low bands x5 loses its leading
// terms (they cancel to about (1 - E)^2), and an ulp more or less in E, cos or sin from one libm to the next then moves an f64 evaluation
// by hundreds of ulps (5e-13 relative at 0 Hz / 16 kHz).  The extended evaluation sits within an ulp or two of the formula's value, which
// every f64 evaluation of it, the reference's included, scatters around.
typedef long double Ld;
struct Cx {
    Ld re, im;
};
Cx cmul(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
Cx cscale(Cx a, Ld s) { return {a.re * s, a.im * s}; }
Cx cadd(Cx a, Cx b) { return {a.re + b.re, a.im + b.im}; }
Cx csub(Cx a, Cx b) { return {a.re - b.re, a.im - b.im}; }

double iir_gain(double cf, double sample_rate) {
    const Ld pi = 3.14159265358979323846264338327950288L;
    const Ld t = 1.0L / Ld(sample_rate);
    const Ld bval = Ld(1.019) * 2.0L * pi * (Ld(cf) / Ld(9.26449) + Ld(24.7));
    const Ld angle = 2.0L * pi * Ld(cf) * t;
    const Ld cos1 = std::cos(angle), sin1 = std::sin(angle);
    const Cx xexp{std::cos(2.0L * angle), std::sin(2.0L * angle)};
    const Ld ebt = std::exp(-bval * t);
    const Cx x01 = cscale(xexp, -2.0L * t);
    const Cx x02 = cscale(Cx{cos1, sin1}, 2.0L * t * ebt);
    const Ld s1 = std::sqrt(3.0L - 2.0L * std::sqrt(2.0L)), s2 = std::sqrt(3.0L + 2.0L * std::sqrt(2.0L));
    const Cx x1 = cadd(x01, cscale(x02, cos1 - s1 * sin1));
    const Cx x2 = cadd(x01, cscale(x02, cos1 + s1 * sin1));
    const Cx x3 = cadd(x01, cscale(x02, cos1 - s2 * sin1));
    const Cx x4 = cadd(x01, cscale(x02, cos1 + s2 * sin1));
    const Ld e2 = ebt * ebt;
    const Cx x5 = cadd(csub(Cx{-2.0L * e2, 0.0L}, cscale(xexp, 2.0L)), cscale(cadd(Cx{1.0L, 0.0L}, xexp), 2.0L * ebt));
    const Cx num = cmul(cmul(cmul(x1, x2), x3), x4);
    const Cx sq = cmul(x5, x5), den = cmul(sq, sq);
    const Ld n2 = den.re * den.re + den.im * den.im;
    const Cx qt{(num.re * den.re + num.im * den.im) / n2, (num.im * den.re - num.re * den.im) / n2};
    return double(std::hypot(qt.re, qt.im));
}

// make_iir_bank (src/erb.rs:456-497): per band a0_1 / gain, a1_1 / gain, a0_2, a1_2, a0_3, a1_3, a0_4, a1_4, b1, b2, gain
void build_bank(const std::vector<double> &centres, double sample_rate, std::vector<double> &coef) {
    const double t = 1.0 / sample_rate;
    coef.resize(centres.size() * kCoef);
    for (size_t m = 0; m < centres.size(); ++m) {
        const double cf = centres[m];
        const double erb = cf / 9.26449 + 24.7;
        const double bval = 1.019 * 2.0 * kPiG * erb;
        const double ebt = std::exp(-bval * t);
        const double angle = 2.0 * kPiG * cf * t;
        const double cos1 = std::cos(angle), sin1 = std::sin(angle);
        const double b1 = -2.0 * cos1 * ebt, b2 = std::exp(-2.0 * bval * t);
        const double s1 = std::sqrt(3.0 - 2.0 * std::sqrt(2.0)), s2 = std::sqrt(3.0 + 2.0 * std::sqrt(2.0));
        const double bsin = sin1 * t;
        const double a11 = -ebt * (t * cos1 + bsin * s2), a12 = -ebt * (t * cos1 - bsin * s2);
        const double a13 = -ebt * (t * cos1 + bsin * s1), a14 = -ebt * (t * cos1 - bsin * s1);
        const double gain = iir_gain(cf, sample_rate);
        double *c = &coef[m * kCoef];
        c[0] = t / gain; c[1] = a11 / gain;
        c[2] = t; c[3] = a12;
        c[4] = t; c[5] = a13;
        c[6] = t; c[7] = a14;
        c[8] = b1; c[9] = b2; c[10] = gain;
    }
}

size_t frames_of(const sgx_gammatone *p, size_t n_samples) { return 1 + (n_samples - p->frame) / p->hop; }

sgx_status run_dev(sgx_gammatone *p, const void *in, size_t batch, size_t stride, size_t n_frames, void *out, hipStream_t s) {
    GtArgs a{};
    a.x = in; a.out = out;
    a.win = p->d_win.as<double>(); a.coef = p->d_coef.as<double>();
    a.sample_stride = stride;
    a.pairs = (unsigned long long)n_frames * p->n_bands;
    a.frame = unsigned(p->frame); a.hop = unsigned(p->hop); a.n_frames = unsigned(n_frames); a.n_bands = unsigned(p->n_bands);
    const unsigned long long wgs = (a.pairs + kGtLanes - 1) / kGtLanes;
    if (wgs * batch >= 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch x frames x bands too large for one launch");
    a.wgs = unsigned(wgs);
    // frames a workgroup's 256 consecutive pairs can touch, and the chunk of each that fits kGtLds beside the others'
    // (a workgroup starts at a multiple of 256, i.e. of g = gcd(256, n_bands), so at most n_bands - g pairs into a frame)
    size_t g = kGtLanes, r = p->n_bands % kGtLanes;
    while (r) { const size_t t = g % r; g = r; r = t; }
    const size_t fmax = std::min<size_t>(n_frames, (p->n_bands - g + kGtLanes - 1) / p->n_bands + 1);
    size_t room = (kGtLds / sizeof(double)) / fmax - 2;
    room = room >= 32 ? room / 32 * 32 : room & ~size_t(1);  // whole bank rows where they fit: the + 2 of the row pitch then shifts the banks
    a.chunk = unsigned(std::min<size_t>(room, (p->frame + 1) & ~size_t(1)));
    a.rstride = a.chunk + 2u;
    a.db = p->db ? 1 : 0;
    a.eps = p->eps; a.floor_val = p->floor_val;
    const size_t lds = fmax * a.rstride * sizeof(double);
    const dim3 grid(unsigned(wgs * batch));
    if (p->dtype == SGX_F64) hipLaunchKernelGGL(k_gammatone_iir<double>, grid, dim3(kGtLanes), lds, s, a);
    else hipLaunchKernelGGL(k_gammatone_iir<float>, grid, dim3(kGtLanes), lds, s, a);
    SGX_TRY_HIP(p, hipGetLastError());
    return SGX_OK;
}

}  // namespace

extern "C" {

sgx_status sgx_gammatone_create(double sample_rate, size_t frame_size, size_t hop_size, uint32_t n_filters, double f_min, double f_max,
                                int32_t erb_spacing, int32_t has_db_floor, double db_floor, int32_t dtype, int32_t device,
                                sgx_gammatone **out) {
    if (out) *out = nullptr;
    if (!out) return fail<sgx_gammatone>(nullptr, SGX_INVALID_INPUT, "Invalid input: null argument");
    auto bad = [&](const char *m) { return fail<sgx_gammatone>(nullptr, SGX_INVALID_INPUT, std::string("Invalid input: ") + m); };
    if (sample_rate <= 0.0) return bad("sample_rate must be > 0");  // src/erb.rs:610-612
    if (!std::isfinite(sample_rate)) return bad("sample_rate must be finite");
    if (frame_size < 2) return bad("frame_size must be >= 2");  // the window divides by frame_size - 1
    if (hop_size == 0) return bad("hop_size must be > 0");
    if (frame_size > 0x7fffffffull || hop_size > 0x7fffffffull) return bad("frame_size or hop_size too large");
    // ErbParams::new src/erb.rs:66-80
    if (n_filters < 2) return bad("n_filters must be >= 2 (single filter would cause division by zero)");
    if (f_min < 0.0 || !std::isfinite(f_min)) return bad("f_min must be finite and >= 0");
    if (!(f_max > f_min)) return bad("f_max must be > f_min");
    if (!std::isfinite(f_max)) return bad("f_max must be finite");
    if (n_filters > kGtMaxFilters) return bad("n_filters is unreasonably large");
    if (erb_spacing != SGX_ERB_LINEAR && erb_spacing != SGX_ERB_APPLE_TR35) return bad("unknown ERB spacing");
    if (has_db_floor && !std::isfinite(db_floor)) return bad("db_floor must be finite");
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    sgx_gammatone *p = new (std::nothrow) sgx_gammatone();
    if (!p) return fail<sgx_gammatone>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->sample_rate = sample_rate; p->frame = frame_size; p->hop = hop_size; p->n_bands = n_filters;
    p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    erb_center_freqs(n_filters, f_min, f_max, erb_spacing, p->centres);
    build_bank(p->centres, sample_rate, p->coef);
    p->window.resize(frame_size);  // hann_window :545-549 (the divisor is frame_size - 1)
    for (size_t i = 0; i < frame_size; ++i) p->window[i] = 0.5 - 0.5 * std::cos(2.0 * kPiG * double(i) / double(frame_size - 1));
    if (has_db_floor) {  // :647-651, in T
        p->db = true;
        const double e = std::pow(10.0, db_floor / 10.0);
        if (dtype == SGX_F64) {
            p->eps = e;
            p->floor_val = 10.0 * std::log10(e);
        } else {
            const float ef = float(e);
            p->eps = double(ef);
            p->floor_val = double(10.0f * std::log10(ef));
        }
    }
    if (device == -2) { *out = p; return SGX_OK; }  // host-only: validation, shapes, centre frequencies, coefficients, route

    auto tables = [&]() -> sgx_status {
        if (device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        const sgx_status st = upload(p, p->d_win, p->window, SGX_F64);  // the recurrences run in f64 for both types
        return st != SGX_OK ? st : upload(p, p->d_coef, p->coef, SGX_F64);
    };
    return finish_create(p, tables(), out, sgx_gammatone_destroy);
}

void sgx_gammatone_destroy(sgx_gammatone *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    delete p;
}

sgx_status sgx_gammatone_output_shape(const sgx_gammatone *p, size_t n_samples, size_t *n_bands, size_t *n_frames) {
    if (!p || !n_bands || !n_frames) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (n_samples < p->frame) return fail(p, SGX_INVALID_INPUT, "Invalid input: signal is shorter than frame_size");  // src/erb.rs:616-620
    *n_bands = p->n_bands;
    *n_frames = frames_of(p, n_samples);
    return SGX_OK;
}

sgx_status sgx_gammatone_execute(sgx_gammatone *p, const void *samples, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                                 size_t out_elems, int32_t mem_kind, void *hip_stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!samples || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    size_t nb, nf;
    sgx_status st = sgx_gammatone_output_shape(p, n_samples, &nb, &nf);
    if (st != SGX_OK) return st;
    if (sample_stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride must be >= n_samples");
    if (batch > 0x7fffffffull || nf > 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or frame count too large");
    const size_t expected = batch * nb * nf;
    if (out_elems != expected)
        return dim_mismatch(p, expected, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return run_dev(p, samples, batch, sample_stride, nf, out, s);
    if (mem_kind != SGX_MEM_HOST) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    // host rows are staged densely (row stride n_samples on the device)
    const size_t row_bytes = n_samples * p->elem, out_bytes = expected * p->elem;
    if ((st = grow(p, p->d_in, batch * row_bytes)) != SGX_OK) return st;
    if ((st = grow(p, p->d_out, out_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpy2DAsync(p->d_in, row_bytes, samples, sample_stride * p->elem, row_bytes, batch, hipMemcpyHostToDevice, s));
    if ((st = run_dev(p, p->d_in, batch, n_samples, nf, p->d_out, s)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

sgx_status sgx_gammatone_center_frequencies(const sgx_gammatone *p, double *out) {
    if (!p || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::memcpy(out, p->centres.data(), p->centres.size() * sizeof(double));
    return SGX_OK;
}

sgx_status sgx_gammatone_coefficients(const sgx_gammatone *p, double *out) {
    if (!p || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::memcpy(out, p->coef.data(), p->coef.size() * sizeof(double));
    return SGX_OK;
}

sgx_status sgx_gammatone_reserve(sgx_gammatone *p, size_t batch, size_t n_samples, int32_t host_staging) {
    if (!p || batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    size_t nb, nf;
    sgx_status st = sgx_gammatone_output_shape(p, n_samples, &nb, &nf);
    if (st != SGX_OK) return st;
    if (!host_staging) return SGX_OK;
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if ((st = grow(p, p->d_in, batch * n_samples * p->elem)) != SGX_OK) return st;
    return grow(p, p->d_out, batch * nb * nf * p->elem);
}

const char *sgx_gammatone_kernel_name(const sgx_gammatone *p) { return p ? "k_gammatone_iir" : ""; }

int32_t sgx_gammatone_device(const sgx_gammatone *p) { return p ? p->device : -2; }

const char *sgx_gammatone_last_error(const sgx_gammatone *p) { return p ? p->err.c_str() : create_err<sgx_gammatone>().c_str(); }

}  // extern "C"

// resample.hip — batched sample-rate conversion plans (sgx_resample_*) of libspectro_hip.so, kernels and host side.
//
// Not in the reference (its surface has no resampler); the semantics are those of torchaudio.functional.resample, restated without
// its padding of every phase kernel to 2 width + orig taps.  With g = gcd(orig, new), M = orig / g (down), L = new / g (up),
// base = min(L, M) rolloff:
//   phi(t) = sinc(t) w(t / lpw) for |t| < lpw, 0 otherwise;   w(u) = cos^2(pi u / 2) (hann) | I0(beta sqrt(1 - u^2)) / I0(beta) (kaiser)
//   y[m]   = (base / M) sum_n x[n] phi(base (n / M - m / L)),   0 <= m < ceil(n_samples L / M),   x = 0 outside the row
// Polyphase form, m = q L + p:   y[q L + p] = sum_{k < K} c[p][k] x[q M + j0(p) + k]
//   j0(p) the smallest j with |base (j / M - p / L)| < lpw (decided in f64), K the largest support count over p,
//   c[p][k] = (base / M) phi(base ((j0(p) + k) / M - p / L)), built in f64, rounded once to T; exactly 0 beyond the support.
// M = L = 1 is the identity (K = 1, c = [[1]], j0 = [0]).
// Arithmetic: every output is ONE chain in T, acc = 0, then acc = fma(c[p][k], x[..], acc) for k = 0 .. K - 1 ascending, on both
// routes, explicit fma (contraction is not left to the compiler), every tap of the chain taken (a zero sample adds exactly 0).  So
// the bits of an output do not depend on the route, the tiling or the cut of a stream into calls, and an output's error is relative
// to its own K samples: the direct form is what the per-sample bound of tests/test_resample.py needs (fir.hip's header
// records why an FFT form does not meet such a bound); as framing + GEMM on the matrix cores the 44.1 -> 16 kHz table would be the
// padded 475 x 160 block, about 13 times the multiply-adds of the sparse form.
//
// Routes:
//   k_resample_pp<T, KB>  the tuned route, within its budget: K <= 64 (the coefficient registers of a work item, KB = K rounded up to a
//                         multiple of 8), L <= 512 (the work items of a workgroup) and a tile's samples within kPpLds = 64 KiB of
//                         LDS (aimed at kPpLdsAim = 32 KiB, so that several workgroups share a CU).  With K <= 64 the ratio M / L is
//                         below ~5.3 at the default width, and the tile below 23 KiB: the caps that bind are K and L.
//                         A workgroup takes one row's tile of Q = G W consecutive q-blocks (G = max(1, 256 / L) work-item groups,
//                         W <= 16 steps) = Q L consecutive outputs, and stages the (Q - 1) M + (max j0 - min j0) + K samples they read
//                         in LDS: the history left of the row start (streaming) or zeros, zeros right of its end; tiles inside the
//                         row take no range checks and all their loads are in flight at once.  Work item (g, p) owns phase p: it loads c[p][0 .. K) once into registers
//                         (from the [K][L] transposed table: lanes along p read consecutive words) and walks q = g, g + G, .., two
//                         outputs per step: a multiply-add costs one LDS sample read at an immediate offset and no coefficient read.  Lanes run along
//                         m = q L + p, so a wave stores consecutive outputs.  Neighbouring tiles share K - 1 samples: xcd_map.h
//                         keeps them in one XCD.
//                         LDS banks: lanes along p read samples about M / L apart.  M <= L (up-sampling, 16 -> 48 kHz, 44.1 -> 48 kHz)
//                         is conflict-free (equal addresses broadcast); L = 1 with odd M (48 -> 16 kHz: stride 3) too; L = 1 with
//                         even M (32 -> 16 kHz) is 2-way; 44.1 -> 16 kHz (stride 2.76) spreads 32 lanes over 88 words, about 3-way.
//                         Left as it is: see DESIGN.md for what it costs and what would remove it.
//   resample_generic      every other table (and any ratio when asked for): k_resample_generic<T>, one work item per output, table
//                         [L][K] and samples from global memory.  L K above kMaxTable = 2^22 entries is SGX_INVALID_INPUT.
// Streaming: the device holds each row's last K - 1 samples in the first of two plan-owned buffers; k_resample_hist writes the next
// history into the second and k_resample_hist_set copies it back on the stream, so no launch reads what it writes (as k_fir_hist);
// reset and flush zero the first buffer with the same kernel, so a streaming call enqueues launches only.  The host holds N
// (samples consumed) and E (outputs emitted); window starts rise with m, so after a push E = #{m : floor(m / L) M + j0(m mod L) + K - 1
// <= N - 1} is a prefix of the outputs and the first output still owed starts no earlier than N - (K - 1).
#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "plan_host.h"
#include "xcd_map.h"

using namespace sgx;

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr double kPiR = 3.14159265358979323846264338327950288;
constexpr size_t kPpLds = 64 * 1024, kPpLdsAim = 32 * 1024;  // LDS per workgroup of k_resample_pp: the budget, and what a tile aims at
constexpr unsigned kPpMaxTaps = 64, kPpMaxPhases = 512, kPpMaxWalk = 16;
constexpr size_t kMaxTable = size_t(1) << 22;  // entries of the [L][K] table
constexpr u64 kMaxRate = 1ull << 30;           // reduced rates

struct RsArgs {
    const void *x;      // [batch][sample_stride] T: stream positions [N0, N0 + n_samples); not read when n_samples == 0
    void *out;          // [batch][n_out] T: outputs [m0, m0 + n_out)
    const void *hist;   // [batch][K - 1] T: positions [N0 - (K - 1), N0); nullptr: zeros
    const void *tab;    // k_resample_pp: [K][L] T; k_resample_generic: [L][K] T
    const unsigned *j0; // [L]: j0(p) - jmin
    u64 sample_stride, n_samples, n_out, m0;
    i64 N0, jmin;
    unsigned batch, L, M, K, jspan;  // jspan = max j0 - min j0
    unsigned G, W, tiles;            // k_resample_pp: work-item groups, steps per work item, tiles per row
    u64 qa;                          // k_resample_pp: the q-block of output m0 (tile t starts at q-block qa + t G W)
};

__device__ __forceinline__ float fma_t(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return fma(a, b, c); }

// the sample at position r relative to x[0]: the history left of it (zeros beyond its K - 1 samples), zeros right of the row's end
template <typename T>
__device__ __forceinline__ T rs_sample(const T *x, const T *hist, unsigned H, u64 n, i64 r) {
    if (r < 0) return (hist && r >= -(i64)H) ? hist[(i64)H + r] : T(0);
    return (u64)r < n ? x[r] : T(0);
}

template <typename T, int KB>
__global__ __launch_bounds__(512) void k_resample_pp(RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *s = (T *)smem;  // [(nq - 1) M + jspan + K] samples, KB - K words of padding behind them
    const unsigned tid = threadIdx.x;
    const unsigned nblk = a.tiles * a.batch;
    const unsigned lb = xcd_logical_block(nblk);  // neighbouring tiles share K - 1 samples: keep them in one XCD
    if (lb >= nblk) return;
    const unsigned t = lb % a.tiles, b = lb / a.tiles;
    const unsigned K = a.K, H = K - 1u;
    const u64 m1 = a.m0 + a.n_out;
    const u64 q0 = a.qa + (u64)t * (a.G * a.W);
    const unsigned nq = (unsigned)min((u64)(a.G * a.W), (m1 + a.L - 1u) / a.L - q0);  // q-blocks of this tile (>= 1)
    const unsigned span = (nq - 1u) * a.M + a.jspan + K;
    const i64 r0 = (i64)(q0 * a.M) + a.jmin - a.N0;  // s[0] relative to x[0]
    const T *x = a.n_samples ? (const T *)a.x + (size_t)b * a.sample_stride : nullptr;
    const T *hist = a.hist ? (const T *)a.hist + (size_t)b * H : nullptr;
    const unsigned p = tid % a.L, g = tid / a.L;
    const bool active = g < a.G;
    T c[KB];
    if (active) {
        const T *tab = (const T *)a.tab + p;
#pragma unroll
        for (int k = 0; k < KB; ++k) c[k] = k < (int)K ? tab[(size_t)k * a.L] : T(0);
    }
    // The tile inside the row: kStage loads (128 bytes) in flight per work item, a 32 KiB tile in one round of a 256-item workgroup.
    // A workgroup has nothing else to do until its samples are there, so rounds of fewer loads are rounds of memory latency.
    constexpr unsigned kStage = 128 / sizeof(T);
    if (r0 >= 0 && (u64)r0 + span <= a.n_samples) {
        const T *xs = x + r0;
        for (unsigned i0 = tid; i0 < span; i0 += kStage * blockDim.x) {
            T v[kStage];
#pragma unroll
            for (unsigned u = 0; u < kStage; ++u) {
                const unsigned i = i0 + u * blockDim.x;
                v[u] = i < span ? xs[i] : T(0);
            }
#pragma unroll
            for (unsigned u = 0; u < kStage; ++u) {
                const unsigned i = i0 + u * blockDim.x;
                if (i < span) s[i] = v[u];
            }
        }
    } else {
        for (unsigned i = tid; i < span; i += blockDim.x) s[i] = rs_sample(x, hist, H, a.n_samples, r0 + (i64)i);
    }
    __syncthreads();
    if (!active) return;
    const unsigned jo = a.j0[p];
    T *out = (T *)a.out + (size_t)b * a.n_out;
    const i64 rel0 = (i64)(q0 * a.L) - (i64)a.m0;  // output (q0 + qi) L + p of the stream is out[rel0 + qi L + p]
    // two outputs of the phase per step: independent chains, the same coefficient registers.  The last 8 taps of the KB registers may
    // lie beyond K: the chain ends at K (a select, not a zero coefficient: 0 x NaN), and the LDS words such a tap names belong to
    // the tile's padding (pp_span), so the step is straight-line code and its LDS reads can all be in flight
    for (unsigned qi = g; qi < nq; qi += 2u * a.G) {
        const unsigned qj = qi + a.G;
        const bool two = qj < nq;
        const T *sp0 = s + (size_t)qi * a.M + jo, *sp1 = two ? s + (size_t)qj * a.M + jo : sp0;
        // 8 taps of both chains at a time, the next 8 samples of each in flight under them.  The empty asm pins that order: left
        // alone, the compiler either issues every read of the step up front and sinks the chains into the store's branch (3 KB
        // registers), or issues each read of the last 8 taps right in front of its select (16 LDS round trips in a row)
        T acc0 = T(0), acc1 = T(0), u0[8], u1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            u0[j] = sp0[j];
            u1[j] = sp1[j];
        }
#pragma unroll
        for (int kc = 0; kc < KB; kc += 8) {
            T n0[8], n1[8];
            if (kc + 8 < KB) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    n0[j] = sp0[kc + 8 + j];
                    n1[j] = sp1[kc + 8 + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (kc + 8 < KB) {
                    acc0 = fma_t(c[kc + j], u0[j], acc0);
                    acc1 = fma_t(c[kc + j], u1[j], acc1);
                } else {
                    const bool in = kc + j < (int)K;
                    acc0 = in ? fma_t(c[kc + j], u0[j], acc0) : acc0;
                    acc1 = in ? fma_t(c[kc + j], u1[j], acc1) : acc1;
                }
            }
            asm volatile("" : "+v"(acc0), "+v"(acc1)::"memory");  // no code: these 8 taps are done here, no later read is issued above
            if (kc + 8 < KB) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    u0[j] = n0[j];
                    u1[j] = n1[j];
                }
            }
        }
        const i64 o0 = rel0 + (i64)(qi * a.L + p), o1 = rel0 + (i64)(qj * a.L + p);
        if (o0 >= 0 && (u64)o0 < a.n_out) out[o0] = acc0;  // (the first and the last q-block of a call may be partial)
        if (two && o1 >= 0 && (u64)o1 < a.n_out) out[o1] = acc1;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_resample_generic(RsArgs a) {
    const T *tab = (const T *)a.tab;
    const unsigned K = a.K, H = K - 1u;
    const u64 total = (u64)a.batch * a.n_out;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < total; i += (u64)gridDim.x * 256u) {
        const u64 b = i / a.n_out, m = a.m0 + i % a.n_out;
        const u64 q = m / a.L;
        const unsigned p = (unsigned)(m % a.L);
        const i64 r0 = (i64)(q * a.M) + a.jmin + (i64)a.j0[p] - a.N0;
        const T *x = a.n_samples ? (const T *)a.x + b * a.sample_stride : nullptr;
        const T *hist = a.hist ? (const T *)a.hist + b * H : nullptr;
        const T *c = tab + (size_t)p * K;
        T acc = T(0);
        if (r0 >= 0 && (u64)r0 + K <= a.n_samples) {
            for (unsigned k = 0; k < K; ++k) acc = fma_t(c[k], x[r0 + k], acc);
        } else {
            for (unsigned k = 0; k < K; ++k) acc = fma_t(c[k], rs_sample(x, hist, H, a.n_samples, r0 + (i64)k), acc);
        }
        ((T *)a.out)[i] = acc;
    }
}

// the next history: the last H samples of history | x, into the plan's second buffer
template <typename T>
__global__ __launch_bounds__(256) void k_resample_hist(const T *x, u64 sample_stride, u64 n, const T *hin, T *hout, unsigned H, unsigned batch) {
    const u64 total = (u64)batch * H;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < total; i += (u64)gridDim.x * 256u) {
        const u64 b = i / H;
        const unsigned j = (unsigned)(i % H);
        const i64 m = (i64)n - (i64)H + j;
        hout[i] = m >= 0 ? x[b * sample_stride + (u64)m] : hin[b * H + (u64)((i64)H + m)];
    }
}

// the first history buffer from the second (src) or as zeros (src == nullptr).  A launch, not hipMemcpyAsync / hipMemsetAsync: a
// streaming call is then a chain of kernels only, which a captured graph replays in order
template <typename T>
__global__ __launch_bounds__(256) void k_resample_hist_set(T *h, const T *src, u64 total) {
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < total; i += (u64)gridDim.x * 256u) h[i] = src ? src[i] : T(0);
}

// I0 by its power series (all terms positive: relative error of a few ulp for the arguments a Kaiser window takes)
double bessel_i0(double x) {
    const double h = 0.25 * x * x;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= h / (double(k) * double(k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

}  // namespace

struct sgx_resample {
    u64 orig = 0, fresh = 0;
    size_t M = 1, L = 1, K = 1;
    int lpw = 6, method = SGX_RESAMPLE_SINC_HANN;
    double rolloff = 0.99, beta = 0.0, base = 1.0;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    bool pp = false;
    unsigned G = 0, W = 0, KB = 0;  // k_resample_pp: work-item groups, steps, coefficient registers
    std::vector<double> tab;   // [L][K], the T-valued coefficients
    std::vector<int64_t> j0;   // [L]
    i64 jmin = 0;
    unsigned jspan = 0;
    DevBuf d_tab, d_j0;
    DevBuf d_hist[2];  // [rows][K - 1] T: the history, and where k_resample_hist writes the next one
    DevBuf d_in, d_out;
    size_t rows = 0;          // rows of the stream, fixed by the first push after creation / reset / flush (0: not fixed)
    size_t N = 0, E = 0;      // samples consumed and outputs emitted per row since then
    size_t allocations = 0;   // (re)allocations of the plan's own buffers (history, host staging)
    mutable std::string err;
};

namespace {

size_t out_len(const sgx_resample *p, size_t n) {
    return (size_t)(((unsigned __int128)n * p->L + p->M - 1) / p->M);
}

// E(N): the outputs whose whole window lies in the first N samples
size_t emitted(const sgx_resample *p, size_t N) {
    const i64 T = (i64)N - (i64)p->K;  // q M + j0(p) <= T
    size_t e = 0;
    for (size_t ph = 0; ph < p->L; ++ph) {
        const i64 d = T - p->j0[ph];
        if (d >= 0) e += (size_t)(d / (i64)p->M) + 1;
    }
    return e;
}

double phi(const sgx_resample *p, double t) {
    if (!(std::fabs(t) < double(p->lpw))) return 0.0;
    const double u = t / double(p->lpw);
    double w;
    if (p->method == SGX_RESAMPLE_SINC_KAISER) w = bessel_i0(p->beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / bessel_i0(p->beta);
    else { const double c = std::cos(kPiR * u / 2.0); w = c * c; }
    const double a = kPiR * t;
    return (t == 0.0 ? 1.0 : std::sin(a) / a) * w;
}

// t of input sample j for phase ph: base (j / M - ph / L), from the exact integer numerator j L - ph M
double tap_t(const sgx_resample *p, i64 j, size_t ph) {
    const __int128 num = (__int128)j * (__int128)p->L - (__int128)ph * (__int128)p->M;
    return p->base * double(num) / (double(p->M) * double(p->L));
}

sgx_status build_table(sgx_resample *p) {
    const size_t M = p->M, L = p->L;
    if (M == 1 && L == 1) {  // equal rates: the identity
        p->K = 1; p->tab.assign(1, 1.0); p->j0.assign(1, 0); p->jmin = 0; p->jspan = 0;
        return SGX_OK;
    }
    const double hw = double(p->lpw) * double(M) / p->base, scale = p->base / double(M);
    p->j0.resize(L);
    std::vector<uint32_t> cnt(L);
    size_t K = 1;
    for (size_t ph = 0; ph < L; ++ph) {
        const double a = double(M) * double(ph) / double(L);
        const i64 lo = (i64)std::floor(a - hw) - 1, hi = (i64)std::ceil(a + hw) + 1;
        i64 first = hi + 1, last = lo - 1;
        for (i64 j = lo; j <= hi; ++j)
            if (std::fabs(tap_t(p, j, ph)) < double(p->lpw)) { first = std::min(first, j); last = std::max(last, j); }
        if (first > last) return fail(p, SGX_INTERNAL, "Internal error: a phase of the resampling filter has no support");
        p->j0[ph] = first;
        cnt[ph] = uint32_t(last - first + 1);
        K = std::max<size_t>(K, cnt[ph]);
    }
    // window starts must rise with m (the streaming prefix rule)
    for (size_t ph = 1; ph < L; ++ph)
        if (p->j0[ph] < p->j0[ph - 1]) return fail(p, SGX_INTERNAL, "Internal error: phase offsets are not monotone");
    if (p->j0[L - 1] > p->j0[0] + (i64)M) return fail(p, SGX_INTERNAL, "Internal error: phase offsets are not monotone");
    p->K = K;
    p->jmin = p->j0[0];
    p->jspan = unsigned(p->j0[L - 1] - p->j0[0]);
    p->tab.assign(L * K, 0.0);
    for (size_t ph = 0; ph < L; ++ph)
        for (size_t k = 0; k < K; ++k) {
            const double v = scale * phi(p, tap_t(p, p->j0[ph] + (i64)k, ph));
            p->tab[ph * K + k] = p->dtype == SGX_F64 ? v : double(float(v));
        }
    return SGX_OK;
}

// the tuned route's tile: samples of Q = G W q-blocks
// (the KB - K words behind it are named by the taps beyond K, whose values are dropped)
size_t pp_span(const sgx_resample *p, size_t nq) { return (nq - 1) * p->M + p->jspan + p->KB; }

void choose_route(sgx_resample *p, int route) {
    p->pp = false;
    if (route != SGX_RESAMPLE_ROUTE_AUTO || p->K > kPpMaxTaps || p->L > kPpMaxPhases) return;
    p->KB = unsigned((p->K + 7) / 8 * 8);
    p->G = unsigned(std::max<size_t>(1, 256 / p->L));
    unsigned W = kPpMaxWalk;
    while (W > 1 && pp_span(p, size_t(p->G) * W) * p->elem > kPpLdsAim) --W;
    if (pp_span(p, size_t(p->G) * W) * p->elem > kPpLds) return;
    p->W = W;
    p->pp = true;
}

template <typename T>
hipError_t launch_pp_t(const sgx_resample *p, const RsArgs &a, unsigned threads, size_t lds, hipStream_t s) {
    const dim3 grid(xcd_grid((u64)a.tiles * a.batch)), block(threads);
    switch (p->KB) {
#define SGX_RS_CASE(KB) case KB: hipLaunchKernelGGL((k_resample_pp<T, KB>), grid, block, lds, s, a); break;
        SGX_RS_CASE(8) SGX_RS_CASE(16) SGX_RS_CASE(24) SGX_RS_CASE(32) SGX_RS_CASE(40) SGX_RS_CASE(48) SGX_RS_CASE(56) SGX_RS_CASE(64)
#undef SGX_RS_CASE
        default: return hipErrorNotSupported;
    }
    return hipGetLastError();
}

// one call on device pointers: outputs [m0, m0 + n_out) of every row from the samples [N0, N0 + n) (x) and the history (hist)
sgx_status run_dev(sgx_resample *p, const void *x, size_t batch, size_t n, size_t stride, const void *hist, size_t N0, size_t m0, void *out,
                   size_t n_out, hipStream_t s) {
    if (n_out == 0) return SGX_OK;
    RsArgs a{};
    a.x = x; a.out = out; a.hist = p->K > 1 ? hist : nullptr;
    a.tab = p->d_tab; a.j0 = p->d_j0.as<unsigned>();
    a.sample_stride = stride; a.n_samples = n; a.n_out = n_out; a.m0 = m0;
    a.N0 = (i64)N0; a.jmin = p->jmin;
    a.batch = unsigned(batch); a.L = unsigned(p->L); a.M = unsigned(p->M); a.K = unsigned(p->K); a.jspan = p->jspan;
    const bool f64 = p->dtype == SGX_F64;
    if (p->pp) {
        const size_t Q = size_t(p->G) * p->W;
        a.G = p->G; a.W = p->W;
        a.qa = m0 / p->L;
        const u64 nq = (m0 + n_out + p->L - 1) / p->L - a.qa;
        const u64 tiles = (nq + Q - 1) / Q;
        if (tiles * batch >= 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
        a.tiles = unsigned(tiles);
        const size_t lds = pp_span(p, (size_t)std::min<u64>(Q, nq)) * p->elem;
        const unsigned threads = unsigned((p->L * p->G + 63) / 64 * 64);
        SGX_TRY_HIP(p, f64 ? launch_pp_t<double>(p, a, threads, lds, s) : launch_pp_t<float>(p, a, threads, lds, s));
    } else {
        const unsigned grid = grid_for_items((u64)batch * n_out);
        if (f64) hipLaunchKernelGGL(k_resample_generic<double>, dim3(grid), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_resample_generic<float>, dim3(grid), dim3(256), 0, s, a);
        SGX_TRY_HIP(p, hipGetLastError());
    }
    return SGX_OK;
}

sgx_status grow_counted(sgx_resample *p, DevBuf &b, size_t need) {
    if (b.bytes >= need) return SGX_OK;
    ++p->allocations;
    return grow(p, b, need);
}

// the history buffers for `rows` rows; new buffers start as zeros (a call that grows them follows creation, reset or flush)
sgx_status hist_reserve(sgx_resample *p, size_t rows, hipStream_t s) {
    const size_t need = rows * (p->K - 1) * p->elem;
    if (need == 0 || p->d_hist[1].bytes >= need) return SGX_OK;  // ([1] grows last: both are there)
    sgx_status st;
    if ((st = grow_counted(p, p->d_hist[0], need)) != SGX_OK || (st = grow_counted(p, p->d_hist[1], need)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemsetAsync(p->d_hist[0], 0, need, s));
    return SGX_OK;
}

// the first `elems` elements of d_hist[0]: those of d_hist[1] (from_next) or zeros, as one launch on s
hipError_t hist_set(sgx_resample *p, bool from_next, size_t elems, hipStream_t s) {
    if (elems == 0) return hipSuccess;
    const dim3 grid(grid_for_items(elems));
    if (p->dtype == SGX_F64)
        hipLaunchKernelGGL(k_resample_hist_set<double>, grid, dim3(256), 0, s, p->d_hist[0].as<double>(),
                           from_next ? (const double *)p->d_hist[1].as<double>() : nullptr, (u64)elems);
    else
        hipLaunchKernelGGL(k_resample_hist_set<float>, grid, dim3(256), 0, s, p->d_hist[0].as<float>(),
                           from_next ? (const float *)p->d_hist[1].as<float>() : nullptr, (u64)elems);
    return hipGetLastError();
}

enum Mode { WHOLE, PUSH, FLUSH };

// the three compute calls behind their argument checks; the state moves only when everything went out
sgx_status rs_call(sgx_resample *p, Mode mode, const void *x, size_t batch, size_t n, size_t stride, void *out, size_t out_elems,
                   int32_t mem_kind, void *stream) {
    const size_t N0 = mode == WHOLE ? 0 : p->N;
    const size_t m0 = mode == WHOLE ? 0 : p->E;
    const size_t m1 = mode == WHOLE ? out_len(p, n) : mode == PUSH ? emitted(p, N0 + n) : out_len(p, N0);
    const size_t n_out = m1 - m0;
    if (out_elems != batch * n_out) return dim_mismatch(p, batch * n_out, out_elems);
    if (n_out && !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch > 0xffffffffull || n > (size_t(1) << 40) || N0 + n > (size_t(1) << 40) || batch * n_out >= (size_t(1) << 46))
        return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    const size_t H = p->K - 1;
    if (mode == PUSH && (st = hist_reserve(p, batch, s)) != SGX_OK) return st;
    const void *hist = mode == WHOLE || !H ? nullptr : p->d_hist[0].ptr;
    const void *dx = x;
    void *dout = out;
    size_t dstride = stride;
    if (mem_kind == SGX_MEM_HOST) {
        const size_t in_bytes = n ? ((batch - 1) * stride + n) * p->elem : 0, out_bytes = out_elems * p->elem;
        if ((st = grow_counted(p, p->d_in, in_bytes)) != SGX_OK) return st;
        if ((st = grow_counted(p, p->d_out, out_bytes)) != SGX_OK) return st;
        if (in_bytes) SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
        dx = p->d_in; dout = p->d_out;
    }
    if ((st = run_dev(p, dx, batch, n, dstride, hist, N0, m0, dout, n_out, s)) != SGX_OK) return st;
    if (mode == PUSH && H) {
        const unsigned grid = grid_for_items((u64)batch * H);
        if (p->dtype == SGX_F64)
            hipLaunchKernelGGL(k_resample_hist<double>, dim3(grid), dim3(256), 0, s, (const double *)dx, (u64)dstride, (u64)n,
                               p->d_hist[0].as<double>(), p->d_hist[1].as<double>(), unsigned(H), unsigned(batch));
        else
            hipLaunchKernelGGL(k_resample_hist<float>, dim3(grid), dim3(256), 0, s, (const float *)dx, (u64)dstride, (u64)n,
                               p->d_hist[0].as<float>(), p->d_hist[1].as<float>(), unsigned(H), unsigned(batch));
        SGX_TRY_HIP(p, hipGetLastError());
        SGX_TRY_HIP(p, hist_set(p, true, batch * H, s));
    }
    if (mode == FLUSH && H && p->d_hist[0].ptr) SGX_TRY_HIP(p, hist_set(p, false, p->d_hist[0].bytes / p->elem, s));
    if (mem_kind == SGX_MEM_HOST) {
        if (n_out) SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_elems * p->elem, hipMemcpyDeviceToHost, s));
        SGX_TRY_HIP(p, hipStreamSynchronize(s));
    }
    if (mode == PUSH) { p->rows = batch; p->N = N0 + n; p->E = m1; }
    if (mode == FLUSH) { p->rows = 0; p->N = p->E = 0; }
    return SGX_OK;
}

}  // namespace

extern "C" {

sgx_status sgx_resample_create(int64_t orig_freq, int64_t new_freq, int32_t lowpass_filter_width, double rolloff, int32_t method, double beta,
                               int32_t route, int32_t dtype, int32_t device, sgx_resample **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_resample>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out) return bad("null argument");
    if (orig_freq <= 0 || new_freq <= 0) return bad("orig_freq and new_freq must be positive integers");
    if (lowpass_filter_width < 1) return bad("lowpass_filter_width must be >= 1");
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return bad("rolloff must be in (0, 1]");
    if (method != SGX_RESAMPLE_SINC_HANN && method != SGX_RESAMPLE_SINC_KAISER)
        return bad("resampling_method must be sinc_interp_hann or sinc_interp_kaiser");
    if (method == SGX_RESAMPLE_SINC_KAISER && !(std::isfinite(beta) && beta >= 0.0)) return bad("beta must be finite and >= 0");
    if (route != SGX_RESAMPLE_ROUTE_AUTO && route != SGX_RESAMPLE_ROUTE_GENERIC) return bad("unknown route");
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    const u64 g = std::gcd((u64)orig_freq, (u64)new_freq), M = (u64)orig_freq / g, L = (u64)new_freq / g;
    const std::string ratio = std::to_string(M) + " : " + std::to_string(L);
    const double base = double(std::min(M, L)) * rolloff;
    const double kb = (M == 1 && L == 1) ? 1.0 : std::floor(2.0 * lowpass_filter_width * double(M) / base) + 2.0;  // K <= kb
    if (M > kMaxRate || L > kMaxRate || double(L) * kb > double(kMaxTable))
        return bad("the reduced ratio " + ratio + " needs a table of up to " + std::to_string((unsigned long long)(double(L) * kb)) +
                   " coefficients (at most " + std::to_string(kMaxTable) + " are supported)");
    sgx_resample *p = new (std::nothrow) sgx_resample();
    if (!p) return fail<sgx_resample>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->orig = (u64)orig_freq; p->fresh = (u64)new_freq; p->M = M; p->L = L;
    p->lpw = lowpass_filter_width; p->rolloff = rolloff; p->method = method; p->beta = beta; p->base = base;
    p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    sgx_status st = build_table(p);
    if (st == SGX_OK) choose_route(p, route);
    if (st != SGX_OK || device == -2) return finish_create(p, st, out, sgx_resample_destroy);  // host-only: the table and every accessor

    auto tables = [&]() -> sgx_status {
        if (device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        sgx_status s2;
        if (p->pp) {  // [K][L]: lanes along p read consecutive words
            std::vector<double> tr(p->tab.size());
            for (size_t ph = 0; ph < p->L; ++ph)
                for (size_t k = 0; k < p->K; ++k) tr[k * p->L + ph] = p->tab[ph * p->K + k];
            s2 = upload(p, p->d_tab, tr, dtype);
        } else {
            s2 = upload(p, p->d_tab, p->tab, dtype);
        }
        if (s2 != SGX_OK) return s2;
        std::vector<unsigned> rel(p->L);
        for (size_t ph = 0; ph < p->L; ++ph) rel[ph] = unsigned(p->j0[ph] - p->jmin);
        SGX_TRY_HIP(p, hipMalloc(&p->d_j0.ptr, rel.size() * sizeof(unsigned)));
        p->d_j0.bytes = rel.size() * sizeof(unsigned);
        SGX_TRY_HIP(p, hipMemcpy(p->d_j0, rel.data(), p->d_j0.bytes, hipMemcpyHostToDevice));
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_resample_destroy);
}

void sgx_resample_destroy(sgx_resample *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    delete p;
}

sgx_status sgx_resample_resample(sgx_resample *p, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                                 size_t out_elems, int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!x) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || n_samples == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (sample_stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    return rs_call(p, WHOLE, x, batch, n_samples, sample_stride, out, out_elems, mem_kind, stream);
}

sgx_status sgx_resample_process(sgx_resample *p, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                                size_t out_elems, int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!x) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || n_samples == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (sample_stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    if (p->rows && batch != p->rows) return dim_mismatch(p, p->rows, batch, " (rows of the stream; reset() releases them)");
    return rs_call(p, PUSH, x, batch, n_samples, sample_stride, out, out_elems, mem_kind, stream);
}

sgx_status sgx_resample_flush(sgx_resample *p, void *out, size_t out_elems, int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (p->rows == 0) {  // nothing pushed: no launch
        if (out_elems != 0) return dim_mismatch(p, 0, out_elems);
        return SGX_OK;
    }
    return rs_call(p, FLUSH, nullptr, p->rows, 0, 0, out, out_elems, mem_kind, stream);
}

sgx_status sgx_resample_reset(sgx_resample *p, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    p->rows = 0; p->N = p->E = 0;
    if (p->device == -2 || !p->d_hist[0].ptr) return SGX_OK;
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    SGX_TRY_HIP(p, hist_set(p, false, p->d_hist[0].bytes / p->elem, static_cast<hipStream_t>(stream)));
    return SGX_OK;
}

sgx_status sgx_resample_reserve(sgx_resample *p, size_t batch, size_t max_block, int32_t host_staging) {
    if (!p || batch == 0 || max_block == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (p->rows && batch > p->rows) return dim_mismatch(p, p->rows, batch, " (rows of the stream; reset() releases them)");
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    if ((st = hist_reserve(p, batch, nullptr)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipStreamSynchronize(nullptr));
    if (host_staging) {  // a call of max_block samples returns at most out_len(max_block + K) outputs per row, a flush fewer
        if ((st = grow_counted(p, p->d_in, batch * max_block * p->elem)) != SGX_OK) return st;
        if ((st = grow_counted(p, p->d_out, batch * (out_len(p, max_block + p->K) + 1) * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_resample_step(const sgx_resample *p, size_t consumed, size_t n_samples, size_t *n_out, size_t *consumed_after) {
    if (!p || !n_out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (consumed > (size_t(1) << 40) || n_samples > (size_t(1) << 40)) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample count too large");
    const size_t e0 = emitted(p, consumed);
    *n_out = n_samples ? emitted(p, consumed + n_samples) - e0 : out_len(p, consumed) - e0;
    if (consumed_after) *consumed_after = n_samples ? consumed + n_samples : 0;
    return SGX_OK;
}

size_t sgx_resample_out_len(const sgx_resample *p, size_t n_samples) { return p ? out_len(p, n_samples) : 0; }
size_t sgx_resample_up(const sgx_resample *p) { return p ? p->L : 0; }
size_t sgx_resample_down(const sgx_resample *p) { return p ? p->M : 0; }
size_t sgx_resample_taps_per_phase(const sgx_resample *p) { return p ? p->K : 0; }

sgx_status sgx_resample_taps(const sgx_resample *p, double *taps) {
    if (!p || !taps) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->tab.begin(), p->tab.end(), taps);
    return SGX_OK;
}

sgx_status sgx_resample_phase_offsets(const sgx_resample *p, int64_t *offsets) {
    if (!p || !offsets) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->j0.begin(), p->j0.end(), offsets);
    return SGX_OK;
}

size_t sgx_resample_tile(const sgx_resample *p) { return p && p->pp ? size_t(p->G) * p->W * p->L : 0; }
size_t sgx_resample_consumed(const sgx_resample *p) { return p ? p->N : 0; }
size_t sgx_resample_emitted(const sgx_resample *p) { return p ? p->E : 0; }
size_t sgx_resample_allocations(const sgx_resample *p) { return p ? p->allocations : 0; }
const char *sgx_resample_kernel_name(const sgx_resample *p) { return !p ? "" : p->pp ? "k_resample_pp" : "resample_generic"; }
int32_t sgx_resample_device(const sgx_resample *p) { return p ? p->device : -2; }
const char *sgx_resample_last_error(const sgx_resample *p) { return p ? p->err.c_str() : create_err<sgx_resample>().c_str(); }

}  // extern "C"

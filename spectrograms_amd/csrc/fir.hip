// fir.hip — batched overlap-save FIR plans (sgx_fir_*) and regularised spectral deconvolution plans (sgx_deconv_*) of
// libspectro_hip.so, kernels and host side.
//
// Reference: src/convolution.rs (fft_convolve :25-47, fft_deconvolve :60-106, OverlapSaveConvolver :149-270).  With L = taps - 1,
//   y_r[n] = sum_{k < taps} h_r[k] x_r[n - k],   x_r[m] for m < 0 from the row's history (the last L samples of earlier calls)
// Overlap-save with a P-point transform: segment j owns the S = P - L outputs [j S, (j + 1) S) and transforms the P inputs
// e[j S - L, j S - L + P) (e = history | x | zeros); of the circular convolution with h the last S values are alias-free.
// h is real, so one complex sequence could carry TWO segments (z = seg_2p + i seg_2p+1, IFFT(FFT(z) H) = (seg_2p * h) + i (seg_2p+1 * h)).
// A sequence here is ONE segment with a zero imaginary part: in the paired form both parts of every intermediate value carry both
// segments, so a segment's rounding error is relative to the norm of the PAIR, and a quiet segment paired with a loud one (a 10^6 : 1
// level step between them) comes out with 10^3 times the error a transform of its own gives it (an f32 restatement on the CPU,
// DESIGN.md) — outside the per-segment bound the plans are tested against.
//
// Routes:
//   k_fir_os<T, A, B, C>   taps <= 2049: P = A B C in 256 .. 4096 with L <= P / 2.  A workgroup takes a tile of consecutive
//                          segments of one row; pass 1 loads each segment's samples straight into its work items' registers (the history
//                          left of the row start, zeros right of its end; tiles inside the row take no range checks), bs_middle
//                          (bs_middle.h) runs passes 2 and 3, the product with H / P where pass 3 leaves the bins and the same passes
//                          back, and the last pass leaves y[n1 B C + r] in the registers of the work item that loaded
//                          e[n1 B C + r]: lanes along r store S consecutive samples of each segment, nothing is reordered.
//   fir_generic            every taps up to 2^19 (and any taps when asked for): P = next_power_of_two(2 taps), 256 .. 2^20;
//                          k_fir_gather packs the segments into complex scratch, the batched complex dispatch (launch_c2c_any with the
//                          product fused into its store for a shared response; launch_big_c2c above 4096 points, and per-row
//                          responses, with k_fir_mul) runs forward and back, k_fir_scatter stores the alias-free samples; over chunks
//                          of at most kChunkBytes of scratch per buffer.
// The streaming call's next history (the last L samples of history | x) is written by k_fir_hist into the second of two plan-owned
// buffers and copied back on the stream: no launch reads what it writes, and the buffers a call names never change, so a captured
// call replays.
//
// Deconvolution: numerator and denominator rows are zero-padded to n = next_power_of_two(max(n_len, d_len)) and transformed by an
// internal complex-STFT plan of one frame per row (n_fft = hop = n, rectangular window, not centred: sgx_execute is the batched
// R2C, sgx_istft the batched C2R of that length); k_deconv_max reduces max |D_k|^2 per denominator row (one workgroup per row),
// k_deconv_quot forms N conj(D) / (|D|^2 + eps), exactly 0 where that denominator is 0.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "bs_middle.h"
#include "reg_radix.h"
#include "rr_layout.h"
#include "plan_host.h"
#include "xcd_map.h"

using namespace sgx;

namespace {

constexpr double kPiF = 3.14159265358979323846264338327950288;
constexpr size_t kChunkBytes = size_t(256) << 20;  // generic route: scratch per buffer; a call is cut into chunks of sequences
constexpr size_t kFirLds32 = 36 * 1024, kFirLds64 = 72 * 1024;  // LDS per workgroup of k_fir_os, as k_bs_fused (bluestein.hip)
constexpr size_t kMaxFusedTaps = 2049, kMaxTaps = size_t(1) << 19;

struct FirArgs {
    const void *x;     // [batch][sample_stride] T
    void *out;         // [batch][n_out] T
    const void *hist;  // [batch][L] T, nullptr: zero history (the full form)
    const void *H;     // fused: FFT_P(h) / P in the product order of bs_middle, per response row; generic: in natural order
    const void *tw;    // [P] complex T: W_P^k
    unsigned long long sample_stride, n_samples, n_out, h_stride;  // h_stride: complex elements between response rows (0: shared)
    unsigned batch, L, S, nseq, tiles;                            // sequences (segments) per row, tiles per row
};

// sample m of the extended row: the history left of the row start, zeros right of its end
template <typename T>
__device__ __forceinline__ T fir_sample(const T *x, const T *hist, unsigned L, unsigned long long n, long long m) {
    if (m < 0) return hist ? hist[(long long)L + m] : T(0);
    return (unsigned long long)m < n ? x[m] : T(0);
}

// waves per SIMD the register allocation aims at, as k_bs_fused: the same passes with all A points of pass 1 live
template <typename T, int A, int B, int C>
constexpr unsigned fir_waves() {
    if (sizeof(T) == 8 && A == 16 && B * C <= 128) return 2;
    return rr_waves<T, A, B, C>();
}

template <typename T, int A_, int B_, int C_>
__global__ __launch_bounds__(256, (fir_waves<T, A_, B_, C_>())) void k_fir_os(FirArgs a, unsigned ltile) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, B = B_, C = C_, BC = B * C, P = A * BC;
    static_assert(ct_is_pow2(P), "k_fir_os: power-of-two segment lengths");
    typedef RrLayout<sizeof(V), A_, B_, C_> Lay;
    constexpr unsigned FS = Lay::FS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    V *buf = (V *)smem;  // [tile][FS]
    const unsigned tid = threadIdx.x, tile = 1u << ltile;
    const unsigned lb = xcd_logical_block(a.tiles * a.batch);  // neighbouring tiles share the overlap's sample lines: keep them in one XCD
    if (lb >= a.tiles * a.batch) return;
    const unsigned t = lb % a.tiles, b = lb / a.tiles;
    const unsigned p0 = t * tile, ns = min(tile, a.nseq - p0);
    const T *x = (const T *)a.x + (size_t)b * a.sample_stride;
    const T *hist = a.hist ? (const T *)a.hist + (size_t)b * a.L : nullptr;
    const V *Hb = (const V *)a.H + (size_t)b * a.h_stride, *tw = (const V *)a.tw;
    T *out = (T *)a.out + (size_t)b * a.n_out;
    const unsigned L = a.L, S = a.S;
    const unsigned long long n = a.n_samples;
    auto item = [&](unsigned idx, unsigned &s, unsigned &r) {
        r = idx % BC;
        s = idx / BC;
        return idx < tile * BC && s < ns;
    };

    // P1 + T1: z[m] = e[base + m] for m = n1 B C + r, base = p S - L
    for (unsigned idx = tid; idx < tile * BC; idx += 256) {
        unsigned s, r;
        if (!item(idx, s, r)) continue;
        const long long base = (long long)((unsigned long long)(p0 + s) * S) - (long long)L;
        V v[A];
        if (base >= 0 && (unsigned long long)base + P <= n) {  // the segment lies inside the row
            const T *pa = x + base + r;
#pragma unroll
            for (unsigned n1 = 0; n1 < A; ++n1) v[n1] = (V){pa[n1 * BC], T(0)};
        } else {
#pragma unroll
            for (unsigned n1 = 0; n1 < A; ++n1) {
                const long long m = base + (long long)(n1 * BC + r);
                v[n1] = (V){fir_sample(x, hist, L, n, m), T(0)};
            }
        }
        rr_pass1_store<T, A_, B_, C_>(v, buf + (size_t)s * FS, r, tw);
    }
#ifdef SGX_BS_STAMPS
    unsigned long long st_acc[14] = {0}, st_prev = 0;
#endif
    bs_middle<T, A_, B_, C_>(buf, ns, tid, tw, Hb BS_STAMP_ARGS);
    // T1, P1: v[n1] = conj(y[n1 B C + r]), y = seg * h; positions L .. P - 1 are alias-free
    for (unsigned idx = tid; idx < tile * BC; idx += 256) {
        unsigned s, r;
        if (!item(idx, s, r)) continue;
        V v[A];
        rr_pass1_load<T, A_, B_, C_>(v, buf + (size_t)s * FS, r, tw);
        const unsigned long long o0 = (unsigned long long)(p0 + s) * S;
#pragma unroll
        for (unsigned n1 = 0; n1 < A; ++n1) {
            const unsigned m = n1 * BC + r;
            if (m < L) continue;
            const unsigned long long o = o0 + (m - L);  // lanes along r: S consecutive samples per segment
            if (o < a.n_out) out[o] = v[n1].x;
        }
    }
}

// the next history: the last L samples of history | x, into the plan's second buffer
template <typename T>
__global__ __launch_bounds__(256) void k_fir_hist(const T *x, unsigned long long sample_stride, unsigned long long n, const T *hin, T *hout,
                                                  unsigned L, unsigned batch) {
    const unsigned long long total = (unsigned long long)batch * L;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long b = i / L;
        const unsigned j = (unsigned)(i % L);
        const long long m = (long long)n - (long long)L + j;
        hout[i] = m >= 0 ? x[b * sample_stride + (unsigned long long)m] : hin[b * L + (unsigned long long)((long long)L + m)];
    }
}

// ---- generic route ---------------------------------------------------------------------------------------------------------------
// A chunk is `gc` consecutive sequences of the flattened (row, sequence) index q = b nseq + p, starting at q0.
struct FirGen {
    FirArgs f;
    void *seq;  // [gc][P] complex T
    unsigned long long q0, gc;
    unsigned P;
};

template <typename T>
__global__ __launch_bounds__(256) void k_fir_gather(FirGen g) {
    typedef typename PairOf<T>::type V;
    const FirArgs &a = g.f;
    const unsigned long long total = g.gc * g.P;
    V *seq = (V *)g.seq;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long q = g.q0 + i / g.P, b = q / a.nseq, p = q % a.nseq;
        const unsigned m = (unsigned)(i % g.P);
        const T *x = (const T *)a.x + b * a.sample_stride;
        const T *hist = a.hist ? (const T *)a.hist + b * a.L : nullptr;
        const long long pos = (long long)(p * a.S) - (long long)a.L + m;
        seq[i] = (V){fir_sample(x, hist, a.L, a.n_samples, pos), T(0)};
    }
}

// spectra times H / P of the sequence's row (natural order)
template <typename T>
__global__ __launch_bounds__(256) void k_fir_mul(FirGen g) {
    typedef typename PairOf<T>::type V;
    const FirArgs &a = g.f;
    const unsigned long long total = g.gc * g.P;
    V *seq = (V *)g.seq;
    const V *H = (const V *)a.H;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long b = (g.q0 + i / g.P) / a.nseq;
        seq[i] = inreg::cmulv(seq[i], H[b * a.h_stride + i % g.P]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_fir_scatter(FirGen g) {
    typedef typename PairOf<T>::type V;
    const FirArgs &a = g.f;
    const unsigned long long total = g.gc * g.P;
    const V *seq = (const V *)g.seq;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned m = (unsigned)(i % g.P);
        if (m < a.L) continue;
        const unsigned long long q = g.q0 + i / g.P, b = q / a.nseq, p = q % a.nseq;
        const unsigned long long o = p * a.S + (m - a.L);
        T *out = (T *)a.out + b * a.n_out;
        if (o < a.n_out) out[o] = seq[i].x;
    }
}

// ---- deconvolution ---------------------------------------------------------------------------------------------------------------
// max_k |D_k|^2 of each denominator row's half spectrum [rows][nb] (the other half mirrors it): one workgroup per row
template <typename T>
__global__ __launch_bounds__(256) void k_deconv_max(const typename PairOf<T>::type *D, unsigned nb, T *dmax) {
    __shared__ T part[256];
    const typename PairOf<T>::type *row = D + (size_t)blockIdx.x * nb;
    T m = T(0);
    for (unsigned k = threadIdx.x; k < nb; k += 256) {
        const T v = row[k].x * row[k].x + row[k].y * row[k].y;  // norm_sqr
        m = v > m ? v : m;                                       // T::max: a NaN is ignored
    }
    part[threadIdx.x] = m;
    __syncthreads();
    for (unsigned w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] = part[threadIdx.x + w] > part[threadIdx.x] ? part[threadIdx.x + w] : part[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) dmax[blockIdx.x] = part[0];
}

// Q = N conj(D) / (|D|^2 + eps), eps = T(regularization) max |D|^2 of the row, exactly 0 where that denominator is 0; in place over N.
// The DC and Nyquist quotients are real (N and D are there); their imaginary parts are stored as 0.
template <typename T>
__global__ __launch_bounds__(256) void k_deconv_quot(typename PairOf<T>::type *N, const typename PairOf<T>::type *D, const T *dmax, unsigned nb,
                                                     unsigned n, unsigned long long total, unsigned long long d_stride, T reg) {
    typedef typename PairOf<T>::type V;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long b = i / nb;
        const unsigned k = (unsigned)(i % nb);
        const unsigned long long drow = d_stride ? b : 0;
        const V nn = N[i], dd = D[drow * nb + k];
        const T den = (dd.x * dd.x + dd.y * dd.y) + reg * dmax[drow];
        V q = (V){T(0), T(0)};
        if (den != T(0)) q = (V){(nn.x * dd.x + nn.y * dd.y) / den, (nn.y * dd.x - nn.x * dd.y) / den};
        if (k == 0 || 2u * k == n) q.y = T(0);
        N[i] = q;
    }
}

// rows [rows][w_in] -> [rows][w_out]: the first min(w_in, w_out) samples of each row, zeros behind them (the zero padding to n going in,
// the truncation coming out)
template <typename T>
__global__ __launch_bounds__(256) void k_deconv_rows(const T *in, T *out, unsigned long long rows, unsigned long long w_in, unsigned long long w_out) {
    const unsigned long long total = rows * w_out;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long r = i / w_out, c = i % w_out;
        out[i] = c < w_in ? in[r * w_in + c] : T(0);
    }
}

size_t next_pow2(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }

// FFT_P of a real sequence on the host: iterative radix-2, f64
void host_fft(std::vector<double> &re, std::vector<double> &im) {
    const size_t M = re.size();
    for (size_t i = 1, j = 0; i < M; ++i) {
        size_t bit = M >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    std::vector<double> wr(M / 2 + 1), wi(M / 2 + 1);
    for (size_t j = 0; j < M / 2; ++j) {
        const double a = -2.0 * kPiF * double(j) / double(M);
        wr[j] = std::cos(a); wi[j] = std::sin(a);
    }
    for (size_t hh = 1; hh < M; hh <<= 1) {
        const size_t stp = M / (2 * hh);
        for (size_t b0 = 0; b0 < M; b0 += 2 * hh)
            for (size_t j = 0; j < hh; ++j) {
                const double xr = re[b0 + hh + j], xi = im[b0 + hh + j], cr = wr[j * stp], ci = wi[j * stp];
                const double tr = xr * cr - xi * ci, ti = xr * ci + xi * cr;
                const double ur = re[b0 + j], ui = im[b0 + j];
                re[b0 + j] = ur + tr; im[b0 + j] = ui + ti;
                re[b0 + hh + j] = ur - tr; im[b0 + hh + j] = ui - ti;
            }
    }
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_fir {
    size_t taps = 0, ir_rows = 1, block = 0, P = 0, S = 0;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    bool fused = false;
    unsigned fa = 0, fb = 0, fc = 0;
    std::vector<double> ir;  // [ir_rows][taps], rounded to T
    DevBuf d_H, d_tw;
    BigDev big;  // generic route above 4096 points
    DevBuf d_big, d_seq, d_spec, d_in, d_out;
    DevBuf d_hist[2];  // [rows][taps - 1] T: the history, and where k_fir_hist writes the next one
    size_t rows = 0;  // rows of the history, fixed by the first streaming call after creation / reset (0: not fixed)
    mutable std::string err;
};

struct sgx_deconv {
    size_t n_len = 0, d_len = 0, n = 0, nb = 0, out_len = 0;
    double reg = 0.0;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    PlanHandle fft;  // one frame of n samples per row (create_row_fft)
    DevBuf d_num, d_den, d_nspec, d_dspec, d_max, d_in, d_in2, d_out;
    mutable std::string err;
};

namespace {

// The fused route's segment length: next_power_of_two(4 taps) within 256 .. 4096 (taps - 1 <= P / 2 holds for every taps <= 2049)
size_t fused_len(size_t taps) { return std::min<size_t>(4096, std::max<size_t>(256, next_pow2(4 * taps))); }
size_t generic_len(size_t taps) { return std::max<size_t>(256, next_pow2(2 * taps)); }

size_t fused_lds_budget(int dtype) { return dtype == SGX_F64 ? kFirLds64 : kFirLds32; }
size_t fused_seq_bytes(const sgx_fir *p) {
    return rr_seq_bytes(2 * (unsigned)p->elem, p->fa, p->fb, p->fc);
}

template <typename T, int A, int B, int C>
hipError_t launch_os_t(const FirArgs &a, unsigned ltile, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024) {
        const hipError_t e = set_max_dynamic_lds((const void *)k_fir_os<T, A, B, C>, (int)(sizeof(T) == 8 ? kFirLds64 : kFirLds32));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_fir_os<T, A, B, C>), dim3(xcd_grid((unsigned long long)a.tiles * a.batch)), dim3(256), lds, s, a, ltile);
    return hipGetLastError();
}

// the (A, B, C) splits reg_split_len gives the powers of two 256 .. 4096
#define SGX_FIR_SPLITS_F32(X) X(16, 16, 1) X(8, 8, 8) X(16, 8, 8) X(16, 16, 8) X(16, 16, 16)
#define SGX_FIR_SPLITS_F64(X) X(8, 8, 4) X(8, 8, 8) X(16, 8, 8) X(16, 16, 8) X(16, 16, 16)

hipError_t launch_os(const sgx_fir *p, FirArgs a, hipStream_t s) {
    const size_t per = fused_seq_bytes(p), budget = fused_lds_budget(p->dtype);  // per <= budget: sgx_fir_create
    unsigned lt = 4;  // up to 16 sequences per workgroup; no more than the row has
    while (lt > 0 && ((size_t(1) << lt) * per > budget || (1u << (lt - 1)) >= a.nseq)) --lt;
    const unsigned tile = 1u << lt;
    a.tiles = (a.nseq + tile - 1u) / tile;
    const unsigned long long g = (unsigned long long)a.tiles * a.batch;
    if (g == 0 || g >= 0x7fffffffull) return hipErrorInvalidConfiguration;
    const size_t lds = (size_t)tile * per;
    const unsigned fa = p->fa, fb = p->fb, fc = p->fc;
#define SGX_FIR_F32(A, B, C) if (fa == A && fb == B && fc == C) return launch_os_t<float, A, B, C>(a, lt, lds, s);
#define SGX_FIR_F64(A, B, C) if (fa == A && fb == B && fc == C) return launch_os_t<double, A, B, C>(a, lt, lds, s);
    if (p->dtype == SGX_F64) { SGX_FIR_SPLITS_F64(SGX_FIR_F64) } else { SGX_FIR_SPLITS_F32(SGX_FIR_F32) }
#undef SGX_FIR_F32
#undef SGX_FIR_F64
    return hipErrorNotSupported;
}

// generic route: sequences per chunk
size_t gen_chunk(const sgx_fir *p, size_t total_seqs) {
    return std::max<size_t>(1, std::min(total_seqs, kChunkBytes / (p->P * 2 * p->elem)));
}

size_t seqs_of(const sgx_fir *p, size_t n_out) { return (n_out + p->S - 1) / p->S; }  // sequences (segments) per row

sgx_status gen_reserve(sgx_fir *p, size_t total_seqs) {
    const size_t gc = gen_chunk(p, total_seqs), bytes = gc * p->P * 2 * p->elem;
    sgx_status st;
    if ((st = grow(p, p->d_seq, bytes)) != SGX_OK) return st;
    if ((st = grow(p, p->d_spec, bytes)) != SGX_OK) return st;
    if (p->big.M && (st = grow(p, p->d_big, big_scratch_bytes(p->big, p->dtype, gc))) != SGX_OK) return st;
    return SGX_OK;
}

sgx_status run_generic(sgx_fir *p, const FirArgs &a, hipStream_t s) {
    const size_t total = (size_t)a.batch * a.nseq;
    sgx_status st = gen_reserve(p, total);
    if (st != SGX_OK) return st;
    const size_t gc = gen_chunk(p, total);
    const bool f64 = p->dtype == SGX_F64;
    const bool fuse_mul = !p->big.M && p->ir_rows == 1;  // one table for every sequence: the product rides on the forward store
    FirGen g{};
    g.f = a;
    g.P = unsigned(p->P);
    C2cArgs c{};
    c.n = unsigned(p->P);
    while ((1u << c.log2n) < c.n) ++c.log2n;
    c.batch = 1;
    c.in_ss = c.out_ss = p->P;
    c.in_is = c.out_is = 1;
    c.tw = p->d_tw;
    c.scale = 1.0;  // (1 / P is folded into H)
    c.tile = p->big.M ? 0 : fft2d_tile_for(c.n, p->dtype);
    auto transform = [&](const void *in, void *out, int inverse, bool mul) {
        c.in = in; c.out = out; c.inverse = inverse;
        c.mul = mul ? p->d_H : nullptr; c.mul_ks = 1; c.mul_real = 0; c.mul_bcast = 1;
        return p->big.M ? launch_big_c2c(p->big, c, p->d_big, p->dtype, s) : launch_c2c_any(c, p->dtype, s);
    };
    for (size_t q0 = 0; q0 < total; q0 += gc) {
        g.q0 = q0;
        g.gc = std::min(gc, total - q0);
        const unsigned grid = grid_for_items(g.gc * p->P);
        c.nseq = unsigned(g.gc);
        c.tiles = c.tile ? unsigned((g.gc + c.tile - 1) / c.tile) : 0;
        g.seq = p->d_seq;
        if (f64) hipLaunchKernelGGL(k_fir_gather<double>, dim3(grid), dim3(256), 0, s, g);
        else hipLaunchKernelGGL(k_fir_gather<float>, dim3(grid), dim3(256), 0, s, g);
        SGX_TRY_HIP(p, hipGetLastError());
        SGX_TRY_HIP(p, transform(p->d_seq, p->d_spec, 0, fuse_mul));
        if (!fuse_mul) {
            g.seq = p->d_spec;
            if (f64) hipLaunchKernelGGL(k_fir_mul<double>, dim3(grid), dim3(256), 0, s, g);
            else hipLaunchKernelGGL(k_fir_mul<float>, dim3(grid), dim3(256), 0, s, g);
            SGX_TRY_HIP(p, hipGetLastError());
        }
        SGX_TRY_HIP(p, transform(p->d_spec, p->d_seq, 1, false));
        g.seq = p->d_seq;
        if (f64) hipLaunchKernelGGL(k_fir_scatter<double>, dim3(grid), dim3(256), 0, s, g);
        else hipLaunchKernelGGL(k_fir_scatter<float>, dim3(grid), dim3(256), 0, s, g);
        SGX_TRY_HIP(p, hipGetLastError());
    }
    return SGX_OK;
}

// the history buffers for `rows` rows; new buffers start as zeros (a call that grows them follows creation or reset)
sgx_status hist_reserve(sgx_fir *p, size_t rows, hipStream_t s) {
    const size_t need = rows * (p->taps - 1) * p->elem;
    if (need == 0 || p->d_hist[1].bytes >= need) return SGX_OK;  // ([1] grows last: both are there)
    sgx_status st;
    if ((st = grow(p, p->d_hist[0], need)) != SGX_OK || (st = grow(p, p->d_hist[1], need)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemsetAsync(p->d_hist[0], 0, need, s));
    return SGX_OK;
}

sgx_status run_dev(sgx_fir *p, const void *x, size_t batch, size_t n_samples, size_t stride, void *out, size_t n_out, bool streaming,
                   hipStream_t s) {
    const size_t L = p->taps - 1;
    FirArgs a{};
    a.x = x; a.out = out;
    a.hist = streaming && L ? p->d_hist[0].ptr : nullptr;
    a.H = p->d_H; a.tw = p->d_tw;
    a.sample_stride = stride; a.n_samples = n_samples; a.n_out = n_out;
    a.h_stride = p->ir_rows > 1 ? p->P : 0;
    a.batch = unsigned(batch); a.L = unsigned(L); a.S = unsigned(p->S);
    a.nseq = unsigned(seqs_of(p, n_out));
    if (p->fused) {
        SGX_TRY_HIP(p, launch_os(p, a, s));
    } else {
        const sgx_status st = run_generic(p, a, s);
        if (st != SGX_OK) return st;
    }
    if (streaming && L) {
        const unsigned grid = grid_for_items(batch * L);
        if (p->dtype == SGX_F64)
            hipLaunchKernelGGL(k_fir_hist<double>, dim3(grid), dim3(256), 0, s, (const double *)x, stride, n_samples, p->d_hist[0].as<double>(),
                               p->d_hist[1].as<double>(), unsigned(L), unsigned(batch));
        else
            hipLaunchKernelGGL(k_fir_hist<float>, dim3(grid), dim3(256), 0, s, (const float *)x, stride, n_samples, p->d_hist[0].as<float>(),
                               p->d_hist[1].as<float>(), unsigned(L), unsigned(batch));
        SGX_TRY_HIP(p, hipGetLastError());
        SGX_TRY_HIP(p, hipMemcpyAsync(p->d_hist[0], p->d_hist[1], batch * L * p->elem, hipMemcpyDeviceToDevice, s));
    }
    return SGX_OK;
}

sgx_status fir_call(sgx_fir *p, const void *x, size_t batch, size_t n_samples, size_t stride, void *out, size_t out_elems, int32_t mem_kind,
                    void *stream, bool streaming) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!x || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || n_samples == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    if (p->ir_rows > 1 && batch != p->ir_rows)
        return dim_mismatch(p, p->ir_rows, batch, " (the plan holds one impulse response per row)");
    if (streaming && p->rows && batch != p->rows)
        return dim_mismatch(p, p->rows, batch, " (rows of the history; reset() releases them)");
    const size_t n_out = streaming ? n_samples : n_samples + p->taps - 1;
    if (out_elems != batch * n_out)
        return dim_mismatch(p, batch * n_out, out_elems);
    const size_t nseq = seqs_of(p, n_out);
    if (batch > 0xffffffffull || nseq * batch >= 0x7fffffffull || n_samples > (size_t(1) << 40))
        return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    if (streaming && (st = hist_reserve(p, batch, s)) != SGX_OK) return st;
    if (mem_kind == SGX_MEM_DEVICE) {
        st = run_dev(p, x, batch, n_samples, stride, out, n_out, streaming, s);
    } else {
        const size_t in_bytes = ((batch - 1) * stride + n_samples) * p->elem, out_bytes = out_elems * p->elem;
        if ((st = grow(p, p->d_in, in_bytes)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, out_bytes)) != SGX_OK) return st;
        SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
        if ((st = run_dev(p, p->d_in, batch, n_samples, stride, p->d_out, n_out, streaming, s)) != SGX_OK) return st;
        SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
        SGX_TRY_HIP(p, hipStreamSynchronize(s));
    }
    if (st == SGX_OK && streaming) p->rows = batch;
    return st;
}

}  // namespace

extern "C" {

sgx_status sgx_fir_create(const double *ir, size_t taps, size_t ir_rows, size_t block_size, int32_t route, int32_t dtype, int32_t device,
                          sgx_fir **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_fir>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out) return bad("null argument");
    if (taps == 0 || !ir) return bad("impulse response must not be empty");  // src/convolution.rs:172-176
    if (ir_rows == 0) return bad("ir_rows must be > 0");
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    if (route != SGX_FIR_ROUTE_AUTO && route != SGX_FIR_ROUTE_GENERIC) return bad("unknown route");
    if (taps > kMaxTaps)
        return fail<sgx_fir>(nullptr, SGX_BACKEND, "hip -- FFT backend error: an impulse response of " + std::to_string(taps) +
                                                         " taps is not supported (up to 524288)");
    if (ir_rows > 0xffffffffull || ir_rows * generic_len(taps) > (size_t(1) << 28)) return bad("too many impulse responses of this length");
    sgx_fir *p = new (std::nothrow) sgx_fir();
    if (!p) return fail<sgx_fir>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->taps = taps; p->ir_rows = ir_rows; p->block = block_size;
    p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    p->fused = route == SGX_FIR_ROUTE_AUTO && taps <= kMaxFusedTaps;
    p->P = p->fused ? fused_len(taps) : generic_len(taps);
    p->S = p->P - (taps - 1);
    // the fused route needs a pass split whose sequence fits the kernel's LDS (every power of two 256 .. 4096 has one in both types)
    if (p->fused && !(reg_split_len(unsigned(p->P), dtype, &p->fa, &p->fb, &p->fc) && fused_seq_bytes(p) <= fused_lds_budget(dtype))) p->fused = false;
    p->ir.resize(ir_rows * taps);
    for (size_t i = 0; i < ir_rows * taps; ++i) p->ir[i] = dtype == SGX_F64 ? ir[i] : double(float(ir[i]));  // the T-valued taps
    if (device == -2) { *out = p; return SGX_OK; }  // host-only: validation, shapes, route

    auto tables = [&]() -> sgx_status {
        if (device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        const size_t P = p->P;
        // H = FFT_P(h) / P in f64, rounded to T: the fused route in bs_middle's product order ([k3][k1][k2] for bin k1 + A (k2 + B k3),
        // [k2][k1] for the two-pass splits), the generic route in natural order
        std::vector<double> H(2 * ir_rows * P), re(P), im(P);
        for (size_t r = 0; r < ir_rows; ++r) {
            std::fill(re.begin(), re.end(), 0.0);
            std::fill(im.begin(), im.end(), 0.0);
            std::copy(p->ir.begin() + r * taps, p->ir.begin() + (r + 1) * taps, re.begin());
            host_fft(re, im);
            for (size_t k = 0; k < P; ++k) {
                size_t at = k;
                if (p->fused) {
                    const size_t k1 = k % p->fa, k2 = (k / p->fa) % p->fb, k3 = k / (size_t(p->fa) * p->fb);
                    at = p->fc > 1 ? (k3 * p->fa + k1) * p->fb + k2 : k2 * p->fa + k1;
                }
                H[2 * (r * P + at)] = re[k] / double(P);
                H[2 * (r * P + at) + 1] = im[k] / double(P);
            }
        }
        sgx_status st;
        if ((st = upload(p, p->d_H, H, dtype)) != SGX_OK) return st;
        if (P <= 4096) {
            std::vector<double> tw(2 * P);
            for (size_t k = 0; k < P; ++k) {
                const double a = -2.0 * kPiF * double(k) / double(P);
                tw[2 * k] = std::cos(a);
                tw[2 * k + 1] = std::sin(a);
            }
            if ((st = upload(p, p->d_tw, tw, dtype)) != SGX_OK) return st;
        } else {
            BigHost h;
            if (!big_host_tables(unsigned(P), h))
                return fail(p, SGX_BACKEND, "hip -- FFT backend error: no complex transform for length " + std::to_string(P));
            SGX_TRY_HIP(p, big_upload(h, dtype, p->big));
        }
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_fir_destroy);
}

void sgx_fir_destroy(sgx_fir *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    big_free(p->big);
    delete p;
}

sgx_status sgx_fir_process(sgx_fir *p, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                           int32_t mem_kind, void *stream) {
    return fir_call(p, x, batch, n_samples, sample_stride, out, out_elems, mem_kind, stream, true);
}

sgx_status sgx_fir_convolve(sgx_fir *p, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                            int32_t mem_kind, void *stream) {
    return fir_call(p, x, batch, n_samples, sample_stride, out, out_elems, mem_kind, stream, false);
}

sgx_status sgx_fir_reset(sgx_fir *p, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    p->rows = 0;
    if (p->device == -2 || !p->d_hist[0].ptr) return SGX_OK;
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    SGX_TRY_HIP(p, hipMemsetAsync(p->d_hist[0], 0, p->d_hist[0].bytes, static_cast<hipStream_t>(stream)));
    return SGX_OK;
}

sgx_status sgx_fir_reserve(sgx_fir *p, size_t batch, size_t n_samples, int32_t host_staging) {
    if (!p || batch == 0 || n_samples == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (p->rows && batch > p->rows)
        return dim_mismatch(p, p->rows, batch, " (rows of the history; reset() releases them)");
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    if ((st = hist_reserve(p, batch, nullptr)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipStreamSynchronize(nullptr));
    const size_t n_full = n_samples + p->taps - 1;
    if (!p->fused && (st = gen_reserve(p, batch * seqs_of(p, n_full))) != SGX_OK) return st;
    if (host_staging) {
        if ((st = grow(p, p->d_in, batch * n_samples * p->elem)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, batch * n_full * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

size_t sgx_fir_fft_size(const sgx_fir *p) { return p ? p->P : 0; }
size_t sgx_fir_step(const sgx_fir *p) { return p ? p->S : 0; }
size_t sgx_fir_taps(const sgx_fir *p) { return p ? p->taps : 0; }
const char *sgx_fir_kernel_name(const sgx_fir *p) { return !p ? "" : p->fused ? "k_fir_os" : "fir_generic"; }
int32_t sgx_fir_device(const sgx_fir *p) { return p ? p->device : -2; }
const char *sgx_fir_last_error(const sgx_fir *p) { return p ? p->err.c_str() : create_err<sgx_fir>().c_str(); }

// ---- deconvolution ---------------------------------------------------------------------------------------------------------------
sgx_status sgx_deconv_create(size_t n_len, size_t d_len, double regularization, int32_t dtype, int32_t device, sgx_deconv **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_deconv>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out) return bad("null argument");
    if (n_len == 0 || d_len == 0) return bad("numerator and denominator must not be empty");  // NonEmptySlice
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    if (!std::isfinite(regularization)) return bad("regularization must be finite");
    const size_t n = next_pow2(std::max(n_len, d_len));
    if (n > (size_t(1) << 20))
        return fail<sgx_deconv>(nullptr, SGX_BACKEND, "hip -- FFT backend error: a transform of " + std::to_string(n) +
                                                            " points is not supported (up to 1048576)");
    sgx_deconv *p = new (std::nothrow) sgx_deconv();
    if (!p) return fail<sgx_deconv>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->n_len = n_len; p->d_len = d_len; p->n = n; p->nb = n / 2 + 1;
    p->out_len = std::max<size_t>(1, n_len >= d_len ? n_len - d_len + 1 : n_len);
    p->reg = regularization; p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    const sgx_status st = create_row_fft(n, dtype, device, p->fft);
    if (st != SGX_OK) {
        delete p;
        return fail<sgx_deconv>(nullptr, st, sgx_last_create_error());
    }
    p->device = sgx_plan_device(p->fft.get());
    *out = p;
    return SGX_OK;
}

void sgx_deconv_destroy(sgx_deconv *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    delete p;
}

size_t sgx_deconv_output_length(const sgx_deconv *p) { return p ? p->out_len : 0; }

sgx_status sgx_deconv_reserve(sgx_deconv *p, size_t batch, size_t den_rows, int32_t host_staging) {
    if (!p || batch == 0 || (den_rows != 1 && den_rows != batch))
        return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0 and den_rows 1 or batch");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_plan *fft = p->fft.get();
    sgx_status st;
    if ((st = grow(p, p->d_num, batch * p->n * p->elem)) != SGX_OK) return st;
    if ((st = grow(p, p->d_den, den_rows * p->n * p->elem)) != SGX_OK) return st;
    if ((st = grow(p, p->d_nspec, batch * p->nb * 2 * p->elem)) != SGX_OK) return st;
    if ((st = grow(p, p->d_dspec, den_rows * p->nb * 2 * p->elem)) != SGX_OK) return st;
    if ((st = grow(p, p->d_max, den_rows * p->elem)) != SGX_OK) return st;
    if (sgx_reserve(fft, batch, p->n, 0, 0) != SGX_OK || sgx_reserve(fft, batch, p->n, 0, 1) != SGX_OK)
        return fail(p, SGX_BACKEND, sgx_last_error(fft));
    if (host_staging) {
        if ((st = grow(p, p->d_in, batch * p->n_len * p->elem)) != SGX_OK) return st;
        if ((st = grow(p, p->d_in2, den_rows * p->d_len * p->elem)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, batch * p->out_len * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_deconv_execute(sgx_deconv *p, const void *numerator, const void *denominator, size_t batch, size_t den_rows, void *out,
                              size_t out_elems, int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!numerator || !denominator || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || batch > 65535) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be 1 .. 65535");
    if (den_rows != 1 && den_rows != batch)
        return dim_mismatch(p, batch, den_rows, " (denominator rows: 1 or one per numerator row)");
    if (out_elems != batch * p->out_len)
        return dim_mismatch(p, batch * p->out_len, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st = sgx_deconv_reserve(p, batch, den_rows, mem_kind == SGX_MEM_HOST);
    if (st != SGX_OK) return st;
    const size_t es = p->elem, n = p->n, nb = p->nb;
    sgx_plan *fft = p->fft.get();
    const void *num = numerator, *den = denominator;
    void *dst = out;
    if (mem_kind == SGX_MEM_HOST) {
        SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, numerator, batch * p->n_len * es, hipMemcpyHostToDevice, s));
        SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in2, denominator, den_rows * p->d_len * es, hipMemcpyHostToDevice, s));
        num = p->d_in; den = p->d_in2; dst = p->d_out;
    }
    auto rows = [&](const void *in, void *to, size_t nrows, size_t w_in, size_t w_out) {
        if (p->dtype == SGX_F64) hipLaunchKernelGGL(k_deconv_rows<double>, dim3(grid_for_items(nrows * w_out)), dim3(256), 0, s, (const double *)in, (double *)to, nrows, w_in, w_out);
        else hipLaunchKernelGGL(k_deconv_rows<float>, dim3(grid_for_items(nrows * w_out)), dim3(256), 0, s, (const float *)in, (float *)to, nrows, w_in, w_out);
        return hipGetLastError();
    };
    // rows zero-padded to n
    SGX_TRY_HIP(p, rows(num, p->d_num, batch, p->n_len, n));
    SGX_TRY_HIP(p, rows(den, p->d_den, den_rows, p->d_len, n));
    auto fft_fail = [&]() { return fail(p, SGX_BACKEND, sgx_last_error(fft)); };
    if (sgx_execute(fft, p->d_num, batch, n, n, p->d_nspec, batch * nb * 2, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    if (sgx_execute(fft, p->d_den, den_rows, n, n, p->d_dspec, den_rows * nb * 2, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    const unsigned long long total = (unsigned long long)batch * nb, d_stride = den_rows > 1 ? nb : 0;
    if (p->dtype == SGX_F64) {
        hipLaunchKernelGGL(k_deconv_max<double>, dim3(unsigned(den_rows)), dim3(256), 0, s, p->d_dspec.as<inreg::v2d>(), unsigned(nb), p->d_max.as<double>());
        hipLaunchKernelGGL(k_deconv_quot<double>, dim3(grid_for_items(total)), dim3(256), 0, s, p->d_nspec.as<inreg::v2d>(), p->d_dspec.as<inreg::v2d>(),
                           p->d_max.as<double>(), unsigned(nb), unsigned(n), total, d_stride, p->reg);
    } else {
        hipLaunchKernelGGL(k_deconv_max<float>, dim3(unsigned(den_rows)), dim3(256), 0, s, p->d_dspec.as<inreg::v2f>(), unsigned(nb), p->d_max.as<float>());
        hipLaunchKernelGGL(k_deconv_quot<float>, dim3(grid_for_items(total)), dim3(256), 0, s, p->d_nspec.as<inreg::v2f>(), p->d_dspec.as<inreg::v2f>(),
                           p->d_max.as<float>(), unsigned(nb), unsigned(n), total, d_stride, float(p->reg));
    }
    SGX_TRY_HIP(p, hipGetLastError());
    // y = irfft_n(Q) over the padded numerator rows (no longer needed), then the first out_len samples of each row
    if (sgx_istft(fft, p->d_nspec, batch, nb, 1, p->d_num, batch * n, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    SGX_TRY_HIP(p, rows(p->d_num, dst, batch, n, p->out_len));
    if (mem_kind == SGX_MEM_HOST) {
        SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, batch * p->out_len * es, hipMemcpyDeviceToHost, s));
        SGX_TRY_HIP(p, hipStreamSynchronize(s));
    }
    return SGX_OK;
}

int32_t sgx_deconv_device(const sgx_deconv *p) { return p ? p->device : -2; }
const char *sgx_deconv_last_error(const sgx_deconv *p) { return p ? p->err.c_str() : create_err<sgx_deconv>().c_str(); }

}  // extern "C"

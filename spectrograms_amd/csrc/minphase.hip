// minphase.hip — batched minimum-phase FIR conversion plans (sgx_minphase_*) of libspectro_hip.so, kernels and host side.
//
// Reference: src/min_phase.rs (minimum_phase :55-57, minimum_phase_with :67-141), the real-cepstrum method.  Per row, with
// n = next_power_of_two(taps max(oversample, 1)):
//   H = FFT_n(h zero-padded);   eps = 1e-20 max_k |H_k|^2 (1e-300 if that maximum is 0);   L_k = 0.5 ln(|H_k|^2 + eps)
//   c = IFFT_n(L);   folded: c_0 and c_{n/2} kept, c_1 .. c_{n/2-1} doubled, everything above n/2 dropped ([1] for n = 1, [1, 1] for n = 2)
//   C = FFT_n(folded c);   Hmin_k = exp(Re C_k) (cos Im C_k + i sin Im C_k);   y = Re IFFT_n(Hmin), its first min(out_len, n) samples
//
// The arithmetic is f64 for both dtypes: the plan's dtype T is the type of the input and output rows only.  The reference computes in
// T, and in f32 that is not usable on the function's main input, a linear-phase low-pass with zeros on the unit circle: the log
// amplifies the forward transform's rounding at every spectral null (an f32 restatement against f64 on Hann-windowed sinc low-passes:
// 5e-4 of the peak tap at 64 taps, 0.1 at 512, 0.6 at 4096 taps).  The input is T-valued, every transform, the log, the exp
// and the sin / cos are f64 (as the gammatone plans run f64 recurrences for f32 rows), and the result is rounded to T once.  So there
// is one kernel instantiation, and the f32 and f64 plans differ in their loads and stores only.
//
// All four transforms are real transforms of length n (h and the folded c are real, L is real and even, Hmin is Hermitian), each run
// as a complex transform of M = n / 2 points over z[j] = x[2 j] + i x[2 j + 1]:
//   forward   Z = FFT_M(z);  E_k = (Z_k + conj Z_{M-k}) / 2,  O_k = -i (Z_k - conj Z_{M-k}) / 2;  X_k = E_k + W_n^k O_k,
//             X_{M-k} = conj(E_k - W_n^k O_k)                                         (X_0 = Re Z_0 + Im Z_0, X_M = Re Z_0 - Im Z_0)
//   inverse   the same pair backwards, z = IFFT_M(Z) / M
//
// Routes:
//   k_minphase        n <= 4096: one launch, one workgroup of 256 work items per row, the row in LDS (16 M bytes: 32 KB at n = 4096)
//                     for all four transforms; nothing but the input row and the output row touches HBM.  The forward transform is
//                     decimation in frequency and leaves bin k at slot bitrev(k); the steps between the transforms work on the slot
//                     pairs (bitrev(k), bitrev(M - k)) in place; the inverse is the transposed network and takes the bins from those
//                     slots, so nothing is ever reordered.  Two radix-2 stages are fused per pass over LDS (one single stage when
//                     log2 M is odd), twiddles W_n^k come from a plan-owned f64 table, max |H|^2 is a workgroup reduction.  Every
//                     access is 16 bytes, and the lanes of a wave stay off each other's banks: the pair steps walk the slots in
//                     slot order (not in bin order), and the two passes with the shortest strides rotate the order in which a lane
//                     takes its four points.
//   minphase_generic  n up to 2^20 (and any n when asked for): the library's own f64 R2C / C2R of length n — an internal complex-STFT
//                     plan of one frame per row (n_fft = hop = n, rectangular window, not centred: sgx_execute / sgx_istft, as the
//                     deconvolution plans use them) — with elementwise kernels between the transforms: widen and pad, per-row max,
//                     log, fold, exp, truncate and round to T.  The internal plans transform every n from 1 up, so the forced
//                     generic route has no lower limit.
// Scratch is plan-owned and sized by reserve; no launch reads what it writes, and the buffers a call names never change, so a
// captured call replays.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "plan_host.h"

using namespace sgx;

// the row routine is host and device code: a host executor runs the same text on the CPU
#define SGX_MINPHASE_HD __host__ __device__ __forceinline__

namespace {

typedef double2 cd;
constexpr unsigned kMpThreads = 256;
constexpr size_t kMaxFusedN = 4096, kMaxN = size_t(1) << 20;
constexpr double kPiM = 3.14159265358979323846264338327950288;

SGX_MINPHASE_HD cd mk(double x, double y) { cd r; r.x = x; r.y = y; return r; }
SGX_MINPHASE_HD cd cadd(cd a, cd b) { return mk(a.x + b.x, a.y + b.y); }
SGX_MINPHASE_HD cd csub(cd a, cd b) { return mk(a.x - b.x, a.y - b.y); }
SGX_MINPHASE_HD cd cmul(cd a, cd b) { return mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
SGX_MINPHASE_HD cd cmulc(cd a, cd b) { return mk(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)

// the low `bits` bits of k reversed
SGX_MINPHASE_HD unsigned bitrev(unsigned k, unsigned bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (bits) return __brev(k) >> (32u - bits);
#endif
    unsigned r = 0;
    for (unsigned i = 0; i < bits; ++i) r |= ((k >> i) & 1u) << (bits - 1u - i);
    return r;
}

SGX_MINPHASE_HD double mp_load(const void *row, unsigned i, int f32) { return f32 ? double(((const float *)row)[i]) : ((const double *)row)[i]; }
SGX_MINPHASE_HD void mp_store(void *row, unsigned i, double v, int f32) {
    if (f32) ((float *)row)[i] = float(v);
    else ((double *)row)[i] = v;
}
SGX_MINPHASE_HD double mp_eps(double max2) { return max2 > 0.0 ? max2 * 1e-20 : 1e-300; }
SGX_MINPHASE_HD double mp_fold_weight(unsigned m, unsigned n) { return (m == 0 || 2u * m == n) ? 1.0 : (2u * m < n ? 2.0 : 0.0); }
SGX_MINPHASE_HD cd mp_exp(cd c) {
    const double mag = exp(c.x);
    return mk(mag * cos(c.y), mag * sin(c.y));
}

// ---- the M-point complex transforms over LDS (tw[k] = W_n^k, k < M = n / 2; W_M^j = tw[2 j]) ---------------------------------------
// forward, natural order in, bin k at slot bitrev(k) out: radix-2 decimation in frequency, stage lengths M, M / 2, .. 2
SGX_MINPHASE_HD void fwd_single(cd *z, const cd *tw, unsigned M, unsigned tid) {  // the stage of length M
    const unsigned h = M >> 1;
    for (unsigned t = tid; t < h; t += kMpThreads) {
        const cd u = z[t], v = z[t + h];
        z[t] = cadd(u, v);
        z[t + h] = cmul(csub(u, v), tw[2u * t]);
    }
}
// The passes with q = 1 and q = 4 would put the accesses of the lanes that differ in bits 2 .. 3 (and of the pairs that differ in
// bit 1) on the same LDS banks, four to a bank.  Those lanes take their four points in an order rotated by `rot`, so that every load
// and store instruction of a wave covers each 16-byte bank group once; the values are rotated back in registers.
SGX_MINPHASE_HD unsigned pass_rot(unsigned q, unsigned tid) { return q <= 4u ? ((2u * ((tid >> 1) & 1u) + ((tid >> 2) & 3u)) & 3u) : 0u; }
// v[r] holds point (r + rot) & 3 -> v[k] holds point k
SGX_MINPHASE_HD void unrotate4(cd &v0, cd &v1, cd &v2, cd &v3, unsigned rot) {
    if (rot & 1u) { const cd t = v3; v3 = v2; v2 = v1; v1 = v0; v0 = t; }
    if (rot & 2u) { cd t = v0; v0 = v2; v2 = t; t = v1; v1 = v3; v3 = t; }
}
// v[k] holds point k -> v[r] holds point (r + rot) & 3
SGX_MINPHASE_HD void rotate4(cd &v0, cd &v1, cd &v2, cd &v3, unsigned rot) {
    if (rot & 1u) { const cd t = v0; v0 = v1; v1 = v2; v2 = v3; v3 = t; }
    if (rot & 2u) { cd t = v0; v0 = v2; v2 = t; t = v1; v1 = v3; v3 = t; }
}
// the stages of length Lb and Lb / 2 in one pass: the four points j + {0, q, 2 q, 3 q} of every block, q = Lb / 4
SGX_MINPHASE_HD void fwd_pair(cd *z, const cd *tw, unsigned n, unsigned M, unsigned Lb, unsigned tid) {
    const unsigned q = Lb >> 2, lq = 31u - (unsigned)__builtin_clz(q), step = n >> (lq + 2u), rot = pass_rot(q, tid);
    const unsigned o0 = (rot & 3u) << lq, o1 = ((rot + 1u) & 3u) << lq, o2 = ((rot + 2u) & 3u) << lq, o3 = ((rot + 3u) & 3u) << lq;
    for (unsigned t = tid; t < (M >> 2); t += kMpThreads) {
        const unsigned j = t & (q - 1u), base = ((t >> lq) << (lq + 2u)) + j;
        const cd w1 = tw[j * step], w2 = tw[2u * j * step];  // W_Lb^j, W_{Lb/2}^j
        cd a0 = z[base + o0], a1 = z[base + o1], a2 = z[base + o2], a3 = z[base + o3];
        unrotate4(a0, a1, a2, a3, rot);
        const cd b0 = cadd(a0, a2), b1 = cadd(a1, a3), b2 = cmul(csub(a0, a2), w1);
        const cd d = cmul(csub(a1, a3), w1), b3 = mk(d.y, -d.x);  // W_Lb^(j + q) = -i W_Lb^j
        cd c0 = cadd(b0, b1), c1 = cmul(csub(b0, b1), w2), c2 = cadd(b2, b3), c3 = cmul(csub(b2, b3), w2);
        rotate4(c0, c1, c2, c3, rot);
        z[base + o0] = c0;
        z[base + o1] = c1;
        z[base + o2] = c2;
        z[base + o3] = c3;
    }
}
// inverse (unnormalised), bin k at slot bitrev(k) in, natural order out: the transposed network with conjugate twiddles
SGX_MINPHASE_HD void inv_pair(cd *z, const cd *tw, unsigned n, unsigned M, unsigned Lb, unsigned tid) {
    const unsigned q = Lb >> 2, lq = 31u - (unsigned)__builtin_clz(q), step = n >> (lq + 2u), rot = pass_rot(q, tid);
    const unsigned o0 = (rot & 3u) << lq, o1 = ((rot + 1u) & 3u) << lq, o2 = ((rot + 2u) & 3u) << lq, o3 = ((rot + 3u) & 3u) << lq;
    for (unsigned t = tid; t < (M >> 2); t += kMpThreads) {
        const unsigned j = t & (q - 1u), base = ((t >> lq) << (lq + 2u)) + j;
        const cd w1 = tw[j * step], w2 = tw[2u * j * step];
        cd a0 = z[base + o0], a1 = z[base + o1], a2 = z[base + o2], a3 = z[base + o3];
        unrotate4(a0, a1, a2, a3, rot);
        a1 = cmulc(a1, w2);
        a3 = cmulc(a3, w2);
        const cd b0 = cadd(a0, a1), b1 = csub(a0, a1), b2 = cmulc(cadd(a2, a3), w1);
        const cd d = cmulc(csub(a2, a3), w1), b3 = mk(-d.y, d.x);  // conj(W_Lb^(j + q)) = i conj(W_Lb^j)
        cd c0 = cadd(b0, b2), c1 = cadd(b1, b3), c2 = csub(b0, b2), c3 = csub(b1, b3);
        rotate4(c0, c1, c2, c3, rot);
        z[base + o0] = c0;
        z[base + o1] = c1;
        z[base + o2] = c2;
        z[base + o3] = c3;
    }
}
SGX_MINPHASE_HD void inv_single(cd *z, const cd *tw, unsigned M, unsigned tid) {
    const unsigned h = M >> 1;
    for (unsigned t = tid; t < h; t += kMpThreads) {
        const cd u = z[t], v = cmulc(z[t + h], tw[2u * t]);
        z[t] = cadd(u, v);
        z[t + h] = csub(u, v);
    }
}

// The steps between the transforms walk the pairs (k, M - k) in slot order: work item u takes the even slot 2 u, which holds bin
// k = bitrev(2 u) < M / 2, and the odd slot bitrev(M - k) of its partner, so that neighbouring lanes read neighbouring slots (in bin
// order every lane of a wave would be on one bank); twr[u] = W_n^k is the twiddle table in that order.  Work item 0 takes bins 0 and M
// (both in slot 0) and the bin M / 2, which pairs with itself in slot 1.
struct MpPair {
    unsigned sa, sb;  // slots of Z_k and Z_{M-k}
    cd w;             // W_n^k
};
SGX_MINPHASE_HD MpPair pair_of(const cd *twr, unsigned u, unsigned M, unsigned lm) {
    MpPair p;
    p.sa = u ? 2u * u : 1u;
    p.sb = u ? bitrev(M - bitrev(2u * u, lm), lm) : 1u;
    p.w = u ? twr[u] : mk(0.0, -1.0);  // W_n^(n / 4) = -i
    return p;
}
// X_k and X_{M-k} of the real n-point transform from the packed M-point one, 1 <= k <= M / 2
SGX_MINPHASE_HD void unpack_pair(const cd *z, const MpPair &p, cd &xa, cd &xb) {
    const cd a = z[p.sa], b = z[p.sb];
    const cd E = mk(0.5 * (a.x + b.x), 0.5 * (a.y - b.y)), O = mk(0.5 * (a.y + b.y), -0.5 * (a.x - b.x));
    const cd t = cmul(p.w, O);
    xa = cadd(E, t);
    xb = mk(E.x - t.x, -(E.y - t.y));
}
// and back: the slots of Z_k and Z_{M-k} from X_k and X_{M-k}
SGX_MINPHASE_HD void pack_pair(cd *z, const MpPair &p, cd xa, cd xb) {
    const cd E = mk(0.5 * (xa.x + xb.x), 0.5 * (xa.y - xb.y)), D = mk(0.5 * (xa.x - xb.x), 0.5 * (xa.y + xb.y));
    const cd O = cmulc(D, p.w);
    z[p.sa] = mk(E.x - O.y, E.y + O.x);
    z[p.sb] = mk(E.x + O.y, O.x - E.y);
}

// One row.  `ex.par(f)` runs f(tid) for the 256 work items of the row and then a barrier; z: M complex values, red: 256 + 16 doubles.
template <typename Exec>
SGX_MINPHASE_HD void minphase_row(Exec &ex, cd *z, double *red, const cd *tw, const cd *twr, const void *ir, void *out, unsigned taps, unsigned n,
                                  unsigned out_len, int f32) {
    if (n == 1) {  // one bin: y = sqrt(h^2 + eps), through the same log and exp
        ex.par([&](unsigned tid) {
            if (tid) return;
            const double h = mp_load(ir, 0, f32), m2 = h * h;
            mp_store(out, 0, exp(0.5 * log(m2 + mp_eps(m2))), f32);
        });
        return;
    }
    const unsigned M = n >> 1;
    unsigned lm = 0;
    while ((1u << lm) < M) ++lm;
    const double inv_m = 1.0 / double(M);
    auto forward = [&]() {
        if (lm & 1u) ex.par([&](unsigned tid) { fwd_single(z, tw, M, tid); });
        for (unsigned Lb = (lm & 1u) ? (M >> 1) : M; Lb >= 4u; Lb >>= 2) ex.par([&](unsigned tid) { fwd_pair(z, tw, n, M, Lb, tid); });
    };
    auto inverse = [&]() {
        for (unsigned Lb = 4u; Lb <= ((lm & 1u) ? (M >> 1) : M); Lb <<= 2) ex.par([&](unsigned tid) { inv_pair(z, tw, n, M, Lb, tid); });
        if (lm & 1u) ex.par([&](unsigned tid) { inv_single(z, tw, M, tid); });
    };
    // z[j] = h[2 j] + i h[2 j + 1], zeros behind the taps
    ex.par([&](unsigned tid) {
        for (unsigned j = tid; j < M; j += kMpThreads) {
            const unsigned m = 2u * j;
            z[j] = mk(m < taps ? mp_load(ir, m, f32) : 0.0, m + 1u < taps ? mp_load(ir, m + 1u, f32) : 0.0);
        }
    });
    forward();
    // max_k |H_k|^2 over k = 0 .. M (the other half mirrors it)
    ex.par([&](unsigned tid) {
        double mx = 0.0;
        auto take = [&](double re, double im) {
            const double v = re * re + im * im;
            mx = v > mx ? v : mx;  // T::max: a NaN is ignored
        };
        if (tid == 0) {
            take(z[0].x + z[0].y, 0.0);
            take(z[0].x - z[0].y, 0.0);
        }
        for (unsigned u = tid; u < (M >> 1); u += kMpThreads) {
            const MpPair p = pair_of(twr, u, M, lm);
            cd xa, xb;
            unpack_pair(z, p, xa, xb);
            take(xa.x, xa.y);
            take(xb.x, xb.y);
        }
        red[tid] = mx;
    });
    ex.par([&](unsigned tid) {
        if (tid >= 16u) return;
        double mx = red[16u * tid];
        for (unsigned i = 1; i < 16u; ++i) mx = red[16u * tid + i] > mx ? red[16u * tid + i] : mx;
        red[kMpThreads + tid] = mx;
    });
    // L_k = 0.5 ln(|H_k|^2 + eps), real: packed for the inverse in the slots the pair came from
    ex.par([&](unsigned tid) {
        double mx = red[kMpThreads];
        for (unsigned i = 1; i < 16u; ++i) mx = red[kMpThreads + i] > mx ? red[kMpThreads + i] : mx;
        const double eps = mp_eps(mx);
        if (tid == 0) {
            const double h0 = z[0].x + z[0].y, hm = z[0].x - z[0].y;
            const double l0 = 0.5 * log(h0 * h0 + eps), l1 = 0.5 * log(hm * hm + eps);
            z[0] = mk(0.5 * (l0 + l1), 0.5 * (l0 - l1));
        }
        for (unsigned u = tid; u < (M >> 1); u += kMpThreads) {
            const MpPair p = pair_of(twr, u, M, lm);
            cd xa, xb;
            unpack_pair(z, p, xa, xb);
            const double la = 0.5 * log(xa.x * xa.x + xa.y * xa.y + eps), lb = 0.5 * log(xb.x * xb.x + xb.y * xb.y + eps);
            pack_pair(z, p, mk(la, 0.0), mk(lb, 0.0));
        }
    });
    inverse();
    // c = z / M; folded in place: z[j] holds the samples 2 j and 2 j + 1
    ex.par([&](unsigned tid) {
        for (unsigned j = tid; j < M; j += kMpThreads) {
            const cd v = z[j];
            z[j] = mk(v.x * inv_m * mp_fold_weight(2u * j, n), v.y * inv_m * mp_fold_weight(2u * j + 1u, n));
        }
    });
    forward();
    // Hmin_k = exp(C_k), packed for the inverse (C_0 and C_M are real)
    ex.par([&](unsigned tid) {
        if (tid == 0) {
            const double h0 = exp(z[0].x + z[0].y), hm = exp(z[0].x - z[0].y);
            z[0] = mk(0.5 * (h0 + hm), 0.5 * (h0 - hm));
        }
        for (unsigned u = tid; u < (M >> 1); u += kMpThreads) {
            const MpPair p = pair_of(twr, u, M, lm);
            cd xa, xb;
            unpack_pair(z, p, xa, xb);
            pack_pair(z, p, mp_exp(xa), mp_exp(xb));
        }
    });
    inverse();
    ex.par([&](unsigned tid) {
        for (unsigned j = tid; j < M; j += kMpThreads) {
            const unsigned m = 2u * j;
            if (m < out_len) mp_store(out, m, z[j].x * inv_m, f32);
            if (m + 1u < out_len) mp_store(out, m + 1u, z[j].y * inv_m, f32);
        }
    });
}

struct MpArgs {
    const void *ir;  // [batch][taps] T
    void *out;       // [batch][out_len] T
    const cd *tw;    // [n / 2]: W_n^k
    const cd *twr;   // [n / 4]: W_n^bitrev(2 u), the twiddles of the pair steps in slot order
    unsigned taps, n, out_len;
    int f32;
};

struct MpDevExec {
    template <typename F>
    __device__ __forceinline__ void par(F f) {
        f(threadIdx.x);
        __syncthreads();
    }
};

__global__ __launch_bounds__(256) void k_minphase(MpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    __shared__ double red[kMpThreads + 16];
    const size_t es = a.f32 ? 4 : 8, row = blockIdx.x;
    MpDevExec ex;
    minphase_row(ex, (cd *)mp_smem, red, a.tw, a.twr, (const unsigned char *)a.ir + row * a.taps * es, (unsigned char *)a.out + row * a.out_len * es,
                 a.taps, a.n, a.out_len, a.f32);
}

// ---- generic route: the elementwise steps between the library's transforms (rows of n f64 samples, half spectra of nb = n / 2 + 1 bins)
__global__ __launch_bounds__(256) void k_mp_widen(const void *ir, double *x, unsigned long long rows, unsigned taps, unsigned n, int f32) {
    const unsigned long long total = rows * n;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long r = i / n;
        const unsigned c = (unsigned)(i % n);
        x[i] = c < taps ? (f32 ? double(((const float *)ir)[r * taps + c]) : ((const double *)ir)[r * taps + c]) : 0.0;
    }
}

// max_k |H_k|^2 of each row's half spectrum: one workgroup per row
__global__ __launch_bounds__(256) void k_mp_max(const cd *H, unsigned nb, double *hmax) {
    __shared__ double part[256];
    const cd *row = H + (size_t)blockIdx.x * nb;
    double m = 0.0;
    for (unsigned k = threadIdx.x; k < nb; k += 256) {
        const double v = row[k].x * row[k].x + row[k].y * row[k].y;
        m = v > m ? v : m;
    }
    part[threadIdx.x] = m;
    __syncthreads();
    for (unsigned w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] = part[threadIdx.x + w] > part[threadIdx.x] ? part[threadIdx.x + w] : part[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) hmax[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void k_mp_log(const cd *H, const double *hmax, cd *L, unsigned nb, unsigned long long total) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const cd h = H[i];
        L[i] = mk(0.5 * log(h.x * h.x + h.y * h.y + mp_eps(hmax[i / nb])), 0.0);
    }
}

__global__ __launch_bounds__(256) void k_mp_fold(const double *c, double *f, unsigned n, unsigned long long total) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u)
        f[i] = c[i] * mp_fold_weight((unsigned)(i % n), n);
}

// Hmin = exp(C); the DC and Nyquist bins are real (C is there) and their imaginary parts are stored as 0
__global__ __launch_bounds__(256) void k_mp_exp(const cd *C, cd *Hm, unsigned nb, unsigned n, unsigned long long total) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned k = (unsigned)(i % nb);
        cd h = mp_exp(C[i]);
        if (k == 0 || 2u * k == n) h.y = 0.0;
        Hm[i] = h;
    }
}

__global__ __launch_bounds__(256) void k_mp_out(const double *y, void *out, unsigned n, unsigned out_len, unsigned long long total, int f32) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const double v = y[(i / out_len) * n + i % out_len];
        if (f32) ((float *)out)[i] = float(v);
        else ((double *)out)[i] = v;
    }
}

unsigned mp_grid(unsigned long long total) { return (unsigned)std::max(1ull, std::min((total + 255) / 256, 1ull << 20)); }

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_minphase {
    size_t taps = 0, n = 0, nb = 0, out_len = 0;  // out_len: min(the caller's out_len, n)
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    bool fused = false;
    DevBuf d_tw, d_twr;  // fused: W_n^k [n / 2] and, in the slot order of the pair steps, [n / 4], complex f64
    PlanHandle fft;      // generic: f64, one frame of n samples per row (create_row_fft)
    DevBuf d_x, d_y, d_spec, d_spec2, d_max, d_in, d_out;
    mutable std::string err;
};

namespace {

sgx_status run_fused(sgx_minphase *p, const void *ir, size_t batch, void *out, hipStream_t s) {
    MpArgs a{};
    a.ir = ir; a.out = out; a.tw = p->d_tw.as<cd>(); a.twr = p->d_twr.as<cd>();
    a.taps = unsigned(p->taps); a.n = unsigned(p->n); a.out_len = unsigned(p->out_len);
    a.f32 = p->dtype == SGX_F32;
    const size_t lds = std::max<size_t>(1, p->n / 2) * sizeof(cd);  // <= 32 KB
    hipLaunchKernelGGL(k_minphase, dim3(unsigned(batch)), dim3(kMpThreads), lds, s, a);
    SGX_TRY_HIP(p, hipGetLastError());
    return SGX_OK;
}

sgx_status run_generic(sgx_minphase *p, const void *ir, size_t batch, void *out, hipStream_t s) {
    const size_t n = p->n, nb = p->nb;
    const unsigned long long samples = (unsigned long long)batch * n, bins = (unsigned long long)batch * nb,
                             outs = (unsigned long long)batch * p->out_len;
    const int f32 = p->dtype == SGX_F32;
    double *x = p->d_x.as<double>(), *y = p->d_y.as<double>();
    cd *spec = p->d_spec.as<cd>(), *spec2 = p->d_spec2.as<cd>();
    sgx_plan *fft = p->fft.get();
    auto fft_fail = [&]() { return fail(p, SGX_BACKEND, sgx_last_error(fft)); };
    hipLaunchKernelGGL(k_mp_widen, dim3(mp_grid(samples)), dim3(256), 0, s, ir, x, (unsigned long long)batch, unsigned(p->taps), unsigned(n), f32);
    SGX_TRY_HIP(p, hipGetLastError());
    if (sgx_execute(fft, x, batch, n, n, spec, bins * 2, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    hipLaunchKernelGGL(k_mp_max, dim3(unsigned(batch)), dim3(256), 0, s, (const cd *)spec, unsigned(nb), p->d_max.as<double>());
    hipLaunchKernelGGL(k_mp_log, dim3(mp_grid(bins)), dim3(256), 0, s, (const cd *)spec, p->d_max.as<double>(), spec2, unsigned(nb), bins);
    SGX_TRY_HIP(p, hipGetLastError());
    if (sgx_istft(fft, spec2, batch, nb, 1, y, samples, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    hipLaunchKernelGGL(k_mp_fold, dim3(mp_grid(samples)), dim3(256), 0, s, (const double *)y, x, unsigned(n), samples);
    SGX_TRY_HIP(p, hipGetLastError());
    if (sgx_execute(fft, x, batch, n, n, spec, bins * 2, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    hipLaunchKernelGGL(k_mp_exp, dim3(mp_grid(bins)), dim3(256), 0, s, (const cd *)spec, spec2, unsigned(nb), unsigned(n), bins);
    SGX_TRY_HIP(p, hipGetLastError());
    if (sgx_istft(fft, spec2, batch, nb, 1, y, samples, SGX_MEM_DEVICE, s) != SGX_OK) return fft_fail();
    hipLaunchKernelGGL(k_mp_out, dim3(mp_grid(outs)), dim3(256), 0, s, (const double *)y, out, unsigned(n), unsigned(p->out_len), outs, f32);
    SGX_TRY_HIP(p, hipGetLastError());
    return SGX_OK;
}

}  // namespace

extern "C" {

sgx_status sgx_minphase_create(size_t taps, size_t out_len, size_t oversample, int32_t route, int32_t dtype, int32_t device, sgx_minphase **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_minphase>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out) return bad("null argument");
    if (taps == 0) return bad("impulse response must not be empty");   // src/min_phase.rs:72-76
    if (out_len == 0) return bad("out_len must be greater than zero");  // :77-81
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    if (route != SGX_MINPHASE_ROUTE_AUTO && route != SGX_MINPHASE_ROUTE_GENERIC) return bad("unknown route");
    const size_t os = std::max<size_t>(oversample, 1);
    size_t n = 0;  // 0: above every supported length
    if (taps <= kMaxN && os <= kMaxN) {
        n = 1;
        while (n < taps * os) n <<= 1;
        if (n > kMaxN) n = 0;
    }
    if (n == 0)
        return fail<sgx_minphase>(nullptr, SGX_BACKEND, "hip -- FFT backend error: a transform of next_power_of_two(" + std::to_string(taps) + " x " +
                                               std::to_string(os) + ") points is not supported (up to 1048576)");
    sgx_minphase *p = new (std::nothrow) sgx_minphase();
    if (!p) return fail<sgx_minphase>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->taps = taps; p->n = n; p->nb = n / 2 + 1; p->out_len = std::min(out_len, n);
    p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    p->fused = route == SGX_MINPHASE_ROUTE_AUTO && n <= kMaxFusedN;
    if (device == -2) { *out = p; return SGX_OK; }  // host-only: validation, shapes, route

    auto tables = [&]() -> sgx_status {
        if (p->fused) {
            if (device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
            DeviceGuard dg;
            SGX_TRY_HIP(p, dg.enter(p->device));
            std::vector<double> tw(2 * std::max<size_t>(1, n / 2));
            for (size_t k = 0; k < tw.size() / 2; ++k) {
                const double a = -2.0 * kPiM * double(k) / double(n);
                tw[2 * k] = std::cos(a);
                tw[2 * k + 1] = std::sin(a);
            }
            sgx_status st;
            if ((st = upload(p, p->d_tw, tw, SGX_F64)) != SGX_OK) return st;
            const unsigned M = unsigned(n / 2);
            unsigned lm = 0;
            while ((1u << lm) < M) ++lm;
            std::vector<double> twr(2 * std::max<size_t>(1, M / 2));
            for (unsigned u = 0; u < M / 2; ++u) {
                const unsigned k = bitrev(2u * u, lm);
                twr[2 * u] = tw[2 * k];
                twr[2 * u + 1] = tw[2 * k + 1];
            }
            return upload(p, p->d_twr, twr, SGX_F64);
        }
        const sgx_status st = create_row_fft(n, SGX_F64, device, p->fft);
        if (st != SGX_OK) return fail(p, st, sgx_last_create_error());
        p->device = sgx_plan_device(p->fft.get());
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_minphase_destroy);
}

void sgx_minphase_destroy(sgx_minphase *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    delete p;
}

sgx_status sgx_minphase_reserve(sgx_minphase *p, size_t batch, int32_t host_staging) {
    if (!p || batch == 0 || batch > 65535) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be 1 .. 65535");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    if (!p->fused) {
        if ((st = grow(p, p->d_x, batch * p->n * sizeof(double))) != SGX_OK) return st;
        if ((st = grow(p, p->d_y, batch * p->n * sizeof(double))) != SGX_OK) return st;
        if ((st = grow(p, p->d_spec, batch * p->nb * sizeof(cd))) != SGX_OK) return st;
        if ((st = grow(p, p->d_spec2, batch * p->nb * sizeof(cd))) != SGX_OK) return st;
        if ((st = grow(p, p->d_max, batch * sizeof(double))) != SGX_OK) return st;
        if (sgx_reserve(p->fft.get(), batch, p->n, 0, 0) != SGX_OK || sgx_reserve(p->fft.get(), batch, p->n, 0, 1) != SGX_OK)
            return fail(p, SGX_BACKEND, sgx_last_error(p->fft.get()));
    }
    if (host_staging) {
        if ((st = grow(p, p->d_in, batch * p->taps * p->elem)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, batch * p->out_len * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_minphase_execute(sgx_minphase *p, const void *ir, size_t batch, void *out, size_t out_elems, int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!ir || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0 || batch > 65535) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be 1 .. 65535");
    if (out_elems != batch * p->out_len)
        return dim_mismatch(p, batch * p->out_len, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st = sgx_minphase_reserve(p, batch, mem_kind == SGX_MEM_HOST);
    if (st != SGX_OK) return st;
    const void *src = ir;
    void *dst = out;
    if (mem_kind == SGX_MEM_HOST) {
        SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, ir, batch * p->taps * p->elem, hipMemcpyHostToDevice, s));
        src = p->d_in; dst = p->d_out;
    }
    st = p->fused ? run_fused(p, src, batch, dst, s) : run_generic(p, src, batch, dst, s);
    if (st != SGX_OK) return st;
    if (mem_kind == SGX_MEM_HOST) {
        SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, batch * p->out_len * p->elem, hipMemcpyDeviceToHost, s));
        SGX_TRY_HIP(p, hipStreamSynchronize(s));
    }
    return SGX_OK;
}

size_t sgx_minphase_fft_size(const sgx_minphase *p) { return p ? p->n : 0; }
size_t sgx_minphase_output_length(const sgx_minphase *p) { return p ? p->out_len : 0; }
size_t sgx_minphase_taps(const sgx_minphase *p) { return p ? p->taps : 0; }
const char *sgx_minphase_kernel_name(const sgx_minphase *p) { return !p ? "" : p->fused ? "k_minphase" : "minphase_generic"; }
int32_t sgx_minphase_device(const sgx_minphase *p) { return p ? p->device : -2; }
const char *sgx_minphase_last_error(const sgx_minphase *p) { return p ? p->err.c_str() : create_err<sgx_minphase>().c_str(); }

}  // extern "C"

// welch.hip — batched Welch spectrum estimates (sgx_welch_*) of libspectro_hip.so: the averaged periodogram (PSD), the cross-spectral
// density of two signals (CSD) and their magnitude-squared coherence, kernels and host side.
//
// Semantics (scipy.signal.welch / csd / coherence for real input, nfft = nperseg = n, noverlap = n - hop, average = "mean"): segment s of a
// row holds the samples [s hop, s hop + n), s < m = 1 + (N - n) / hop (no padding, a ragged tail is ignored); each segment is detrended
// (nothing / its mean / its least-squares line), multiplied by the window and transformed, X_s = FFT_n(w (x_s - trend_s)):
//   Pxx[k] = g_k scale mean_s |X_s[k]|^2,   Pxy[k] = g_k scale mean_s conj(X_s[k]) Y_s[k],   C[k] = |Pxy|^2 / (Pxx Pyy)
// with g_k = 2 except g_0 = 1 and g_{n/2} = 1 for even n, scale = 1 / (sample_rate sum w^2) ("density") or 1 / (sum w)^2 ("spectrum").
//
// Routes:
//   k_welch<T, A, B, C, KIND>  n = A B C in 256 .. 4096 (the splits of k_fir_os, fir.hip).  A workgroup takes a tile of `tile` consecutive
//                          segments of one row (of one pair of rows), `sub` of them per round through LDS: pass 1 loads a segment's
//                          samples straight into its work items' registers, forms the segment's sums across the work items that
//                          hold it (the mean in two steps, the slope on the remainders), subtracts the trend BEFORE the window multiply (subtracting mu FFT(w) after the transform
//                          cancels in T under a large DC), then the in-register / LDS passes of the complex transform run on the real
//                          sequence (imaginary part zero).  The two channels of a pair are two such sequences, not one packed x + i y:
//                          packed, a channel's rounding error is relative to the norm of the pair (fir.hip:8-12 has the same finding).
//                          The last pass leaves bins k1 + A (k2 + B k3) in the registers of work item (k1, k2), the same bins for every
//                          segment: |X|^2, |Y|^2 and conj(X) Y are summed there over the tile's segments, never stored per segment.
//                          One partial per tile goes to plan scratch [row][tile][sum][bin]; k_welch_fold adds a row's partials in tile
//                          order and applies g_k scale / m (the quotient for coherence).  No atomics: a row's bits depend on nothing
//                          but its own samples.  Blocks are ordered with xcd_map.h (neighbouring tiles share the overlap's lines).
//   welch_generic          every other n an sgx_plan accepts, and any n when asked for: k_welch_gather writes the detrended, windowed
//                          segments of a chunk to scratch, an internal one-frame-per-row plan (create_row_fft) transforms them,
//                          k_welch_accum adds the chunk's segments to the per-row sums in segment order (so the chunk seams do not
//                          change the bits); chunks of at most max_scratch_bytes per buffer; k_welch_fold finishes.
// The products of the sums are unfused (w_mul / w_add below): conj(X) X has an imaginary part of exactly 0 and the real part of
// |X|^2, and swapping the channels conjugates the cross spectrum bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rr_passes.h"
#include "plan_host.h"
#include "xcd_map.h"

using namespace sgx;

namespace {

constexpr size_t kWelchLdsRound = 72 * 1024;   // LDS of one round's sequences (a pair's two sequences count twice), as k_fir_os
constexpr size_t kWelchLdsMax = 136 * 1024;    // ... but one segment (pair) always fits: f64 n = 4096 needs 2 x 64 KiB
constexpr unsigned kWelchMaxTile = 64;
constexpr size_t kDefaultScratch = size_t(256) << 20;

enum { KIND_PSD = SGX_WELCH_PSD, KIND_CSD = SGX_WELCH_CSD, KIND_COH = SGX_WELCH_COHERENCE };

__host__ __device__ constexpr unsigned welch_nacc(int kind) { return kind == KIND_PSD ? 1u : kind == KIND_CSD ? 2u : 4u; }

struct WelchArgs {
    const void *x, *y;  // [batch][sample_stride] T (y: pair kinds)
    void *part;         // [batch][tiles][nacc][nb] T
    const void *win;    // [n] T
    const void *tw;     // [n] complex T: W_n^k
    unsigned long long sample_stride;
    unsigned batch, hop, nseg, tiles, tile, sub;
    int detrend;
    double inv_n, inv_sxx;  // 1 / n, 1 / sum (j - c)^2 with c = (n - 1) / 2
};

// One rounding per operation, never contracted into an fma (the HIP headers' __fmul_rn / __fadd_rn are plain operators here, which the
// default contraction fuses): conj(X) X must have an imaginary part of exactly 0.
template <typename T>
__device__ __forceinline__ T w_mul(T a, T b) {
#pragma clang fp contract(off)
    return a * b;
}
template <typename T>
__device__ __forceinline__ T w_add(T a, T b) {
#pragma clang fp contract(off)
    return a + b;
}
template <typename T>
__device__ __forceinline__ T w_sub(T a, T b) {
#pragma clang fp contract(off)
    return a - b;
}

// acc += the sums of one bin: [|X|^2] / [Re, Im of conj(X) Y] / [|X|^2, |Y|^2, Re, Im]
template <int KIND, typename T, typename V>
__device__ __forceinline__ void welch_add(T *acc, unsigned stride, V X, V Y) {
    if constexpr (KIND == KIND_PSD) {
        acc[0] = w_add(acc[0], w_add(w_mul(X.x, X.x), w_mul(X.y, X.y)));
    } else {
        const T re = w_add(w_mul(X.x, Y.x), w_mul(X.y, Y.y)), im = w_sub(w_mul(X.x, Y.y), w_mul(X.y, Y.x));
        if constexpr (KIND == KIND_CSD) {
            acc[0] = w_add(acc[0], re);
            acc[stride] = w_add(acc[stride], im);
        } else {
            acc[0] = w_add(acc[0], w_add(w_mul(X.x, X.x), w_mul(X.y, X.y)));
            acc[stride] = w_add(acc[stride], w_add(w_mul(Y.x, Y.x), w_mul(Y.y, Y.y)));
            acc[2 * stride] = w_add(acc[2 * stride], re);
            acc[3 * stride] = w_add(acc[3 * stride], im);
        }
    }
}

template <typename T, int A, int B, int C, int KIND>
constexpr unsigned welch_waves() {
    const unsigned w = rr_waves<T, A, B, C>();
    return KIND == KIND_PSD ? w : (w >= 3 ? 2u : 1u);
}

template <typename T, int A_, int B_, int C_, int KIND>
__global__ __launch_bounds__(256, (welch_waves<T, A_, B_, C_, KIND>())) void k_welch(WelchArgs a) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, B = B_, C = C_, BC = B * C, P = A * BC, NB = P / 2 + 1;
    constexpr unsigned NCH = KIND == KIND_PSD ? 1 : 2, NACC = welch_nacc(KIND);
    constexpr unsigned LAST = C > 1 ? C : B, NBK = LAST / 2 + 1;  // the last pass's points; those at or below n / 2 are kept
    constexpr unsigned Q = C > 1 ? A * B : A, G = 256 / Q;        // work items of the last pass per sequence; threads per item
    constexpr unsigned W = BC < 64 ? BC : 64, WPS = BC / W;       // lanes of a wave, waves, that hold one sequence in pass 1
    constexpr bool kTableTwiddles = sizeof(T) == 8;               // f64: every twiddle read from the table (f32 builds them from LA entries)
    static_assert(ct_is_pow2(P) && 256 % Q == 0 && 256 % BC == 0 && WPS <= 4, "k_welch: power-of-two splits of k_fir_os");
    typedef RrLayout<sizeof(V), A_, B_, C_> Lay;
    constexpr unsigned RS = Lay::RS, FS = Lay::FS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ T red[3][4];  // pass 1, sequences over several waves: the waves' sums, one slot per reduction of an iteration
    V *buf = (V *)smem;         // [sub * NCH][FS]
    const unsigned tid = threadIdx.x;
    const unsigned lb = xcd_logical_block(a.tiles * a.batch);  // neighbouring tiles share the overlap's sample lines: keep them in one XCD
    if (lb >= a.tiles * a.batch) return;
    const unsigned t = lb % a.tiles, b = lb / a.tiles;
    const unsigned p0 = t * a.tile, ns = min(a.tile, a.nseg - p0);
    const T *x = (const T *)a.x + (size_t)b * a.sample_stride;
    const T *y = NCH > 1 ? (const T *)a.y + (size_t)b * a.sample_stride : x;
    const T *win = (const T *)a.win;
    const V *tw = (const V *)a.tw;
    const T inv_n = T(a.inv_n), inv_sxx = T(a.inv_sxx), ctr = T(0.5) * T(P - 1);

    T acc[NACC * NBK];
#pragma unroll
    for (unsigned i = 0; i < NACC * NBK; ++i) acc[i] = T(0);

    for (unsigned s0 = 0; s0 < ns; s0 += a.sub) {
        const unsigned rseg = min(a.sub, ns - s0), nq = rseg * NCH;  // segments, sequences of this round
        // P1 + T1: z[j] = w[j] (x[s hop + j] - trend(j)) for j = n1 B C + r
        const unsigned items = nq * BC, iters = (items + 255u) / 256u;
        for (unsigned it = 0; it < iters; ++it) {
            const unsigned idx = tid + 256u * it, sq = idx / BC, r = idx % BC;
            const bool valid = idx < items;
            T xv[A];
            if (valid) {
                const T *pa = ((sq % NCH) ? y : x) + (size_t)(p0 + s0 + sq / NCH) * a.hop + r;  // (every segment lies inside the row)
#pragma unroll
                for (unsigned n1 = 0; n1 < A; ++n1) xv[n1] = pa[n1 * BC];
            } else {
#pragma unroll
                for (unsigned n1 = 0; n1 < A; ++n1) xv[n1] = T(0);
            }
            if (a.detrend != SGX_WELCH_DETREND_NONE) {  // (uniform)
                // The sum of a value over the work items of the sequence (reduction `slot` of this iteration; every work item ends with
                // the same bits).  A slot's words are rewritten one iteration later, behind the barrier of the slot after it.
                auto seq_sum = [&](T v, unsigned slot) {
#pragma unroll
                    for (unsigned off = 1; off < W; off <<= 1) v += __shfl_xor(v, off, 64);
                    if constexpr (WPS > 1) {
                        const unsigned wv = tid >> 6, w0 = wv / WPS * WPS;
                        if ((tid & 63u) == 0) red[slot][wv] = v;
                        __syncthreads();
                        v = red[slot][w0];
#pragma unroll
                        for (unsigned j = 1; j < WPS; ++j) v += red[slot][w0 + j];
                    }
                    return v;
                };
                // The mean in two steps: under a large offset the first mean is off by a few u |mean|, and that error, times the window,
                // lands on bins 0 and 1 alone (n / 2 times it on bin 0, against a bound that grows like sqrt(n) log n).  The mean of
                // the remainders is small and takes the rest.  The slope is fitted to the remainders for the same reason.
#pragma unroll
                for (unsigned pass = 0; pass < 2; ++pass) {
                    T s = T(0);
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) s += xv[n1];
                    const T mu = seq_sum(s, pass) * inv_n;
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) xv[n1] -= mu;
                }
                if (a.detrend == SGX_WELCH_DETREND_LINEAR) {
                    T s = T(0);
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) s += (T(n1 * BC + r) - ctr) * xv[n1];
                    const T slope = seq_sum(s, 2) * inv_sxx;
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) xv[n1] -= slope * (T(n1 * BC + r) - ctr);
                }
            }
            if (!valid) continue;
            V v[A];
            const T *pw = win + r;
#pragma unroll
            for (unsigned n1 = 0; n1 < A; ++n1) v[n1] = (V){xv[n1] * pw[n1 * BC], T(0)};
            // Pass 1's transform, twiddles and scatter stay written out here (they are rr_pass1_store of rr_passes.h): through the
            // helper the compiler contracts two multiply-adds of k_welch<float, 8, 8, 8, KIND_PSD>'s detrending into fmas that it
            // left as packed multiplies and adds before, and the linear-detrend PSD at n = 512 changes in its last bits.
            constexpr int LA = ct_log2_ceil(A);
            inreg::MixFft<A, V>::run(v);
            V *dst = buf + (size_t)sq * FS;
            const unsigned pp = Lay::hi_part(r / C) ^ (r % C);
            dst[pp ^ Lay::k1_mask(0)] = v[0];
            if constexpr (kTableTwiddles) {  // W^(k1 r) as the table has it: one rounding, against up to LA - 1 products of entries
#pragma unroll
                for (unsigned k1 = 1; k1 < A; ++k1) (dst + (pp ^ Lay::k1_mask(k1)))[k1 * RS] = inreg::cmulv(v[k1], tw[rr_wrap<P>(k1 * r)]);
            } else {
                V pw2[LA];
#pragma unroll
                for (int j = 0; j < LA; ++j) pw2[j] = tw[rr_wrap<P>((1u << j) * r)];
#pragma unroll
                for (unsigned k1 = 1; k1 < A; ++k1) (dst + (pp ^ Lay::k1_mask(k1)))[k1 * RS] = inreg::cmulv(v[k1], rr_twiddle<LA>(pw2, k1));
            }
        }
        __syncthreads();
        if constexpr (C > 1) {
            // P2 + T2: this kernel's own copy of rr_pass2 (rr_passes.h).  With the shared loop k_welch<double, 16, 8, 8, KIND_PSD> goes
            // from 248 to 258 registers, i.e. from two resident workgroups per CU to one (profiles/rr_passes_codegen.txt).
            constexpr int LB = ct_log2_ceil(B);
            for (unsigned idx = tid; idx < nq * A * C; idx += 256) {
                const unsigned sq = idx / (A * C), q = idx % (A * C), k1 = q / C, n3 = q % C;
                V *row = buf + (size_t)sq * FS + k1 * RS;
                const unsigned lp = n3 ^ Lay::k1_mask(k1);
                V v[B];
#pragma unroll
                for (unsigned n2 = 0; n2 < B; ++n2) v[n2] = row[lp ^ Lay::hi_part(n2)];
                inreg::MixFft<B, V>::run(v);
                row[lp ^ Lay::hi_part(0)] = v[0];
                if constexpr (kTableTwiddles) {
#pragma unroll
                    for (unsigned k2 = 1; k2 < B; ++k2) row[lp ^ Lay::hi_part(k2)] = inreg::cmulv(v[k2], tw[rr_wrap<P>(A * k2 * n3)]);
                } else {
                    V q2[LB];
#pragma unroll
                    for (int j = 0; j < LB; ++j) q2[j] = tw[rr_wrap<P>((A << j) * n3)];
#pragma unroll
                    for (unsigned k2 = 1; k2 < B; ++k2) row[lp ^ Lay::hi_part(k2)] = inreg::cmulv(v[k2], rr_twiddle<LB>(q2, k2));
                }
            }
            __syncthreads();
        }
        // the last pass: work item q = tid % Q of every segment holds the bins k1 + A (k2 + B j) (three passes: q = k1 B + k2) or
        // k1 + A j (two passes: q = k1), j < LAST
        for (unsigned idx = tid; idx < rseg * Q; idx += 256) {
            const unsigned s = idx / Q, q = idx % Q;
            const unsigned k1 = C > 1 ? q / B : q;
            const unsigned lp = (C > 1 ? Lay::hi_part(q % B) : 0u) ^ Lay::k1_mask(k1);
            V vx[LAST], vy[LAST];  // (vy: LAST entries also where NCH == 1 leaves it unused, to bind to rr_last_load's array reference)
            const V *rx = buf + (size_t)(s * NCH) * FS + k1 * Lay::RS;
            rr_last_load<T, A_, B_, C_>(vx, rx, lp);
            if constexpr (NCH > 1) rr_last_load<T, A_, B_, C_>(vy, rx + FS, lp);
#pragma unroll
            for (unsigned j = 0; j < NBK; ++j) {
                if constexpr (NCH > 1) welch_add<KIND, T, V>(acc + j, NBK, vx[j], vy[j]);
                else welch_add<KIND, T, V>(acc + j, NBK, vx[j], vx[j]);
            }
        }
        __syncthreads();  // the next round, and the sums below, overwrite the sequences
    }

    // the G threads that share a work item add their sums in thread order; bin k1 + A (k2 + B j) >= n / 2 for j = LAST / 2, with
    // equality at q = 0 only
    T *sums = (T *)smem;  // [NBK][256]
    T *part = (T *)a.part + ((size_t)b * a.tiles + t) * NACC * NB;
#pragma unroll
    for (unsigned c = 0; c < NACC; ++c) {
        if (c) __syncthreads();
#pragma unroll
        for (unsigned j = 0; j < NBK; ++j) sums[j * 256 + tid] = acc[c * NBK + j];
        __syncthreads();
        if (tid < Q) {
#pragma unroll
            for (unsigned j = 0; j < NBK; ++j) {
                T sum = sums[j * 256 + tid];
                for (unsigned g = 1; g < G; ++g) sum = w_add(sum, sums[j * 256 + g * Q + tid]);
                const unsigned k = C > 1 ? tid / B + A * (tid % B + B * j) : tid + A * j;
                if (k < NB) part[c * NB + k] = sum;
            }
        }
    }
}

// out[row][k] from the row's partials [row][tiles][nacc][nb], added in tile order; fac = scale / m
template <typename T>
__global__ __launch_bounds__(256) void k_welch_fold(const T *part, T *out, unsigned nb, unsigned tiles, unsigned n, int kind, double fac,
                                                    unsigned long long total) {
    const unsigned nacc = welch_nacc(kind);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long b = i / nb;
        const unsigned k = (unsigned)(i % nb);
        const T *base = part + b * tiles * nacc * nb + k;
        T s[4] = {T(0), T(0), T(0), T(0)};
        for (unsigned t = 0; t < tiles; ++t)
            for (unsigned c = 0; c < nacc; ++c) s[c] = w_add(s[c], base[((size_t)t * nacc + c) * nb]);
        const T f = T(fac * ((k == 0 || 2u * k == n) ? 1.0 : 2.0));
        if (kind == KIND_PSD) {
            out[i] = w_mul(f, s[0]);
        } else if (kind == KIND_CSD) {
            out[2 * i] = w_mul(f, s[0]);
            out[2 * i + 1] = w_mul(f, s[1]);
        } else {  // |Pxy|^2 / (Pxx Pyy), the scale cancels; as two quotients per part, which neither overflow nor underflow early
            const T a0 = s[2] / s[0], a1 = s[2] / s[1], b0 = s[3] / s[0], b1 = s[3] / s[1];
            out[i] = w_add(w_mul(a0, a1), w_mul(b0, b1));
        }
    }
}

// ---- generic route ---------------------------------------------------------------------------------------------------------------
// A chunk is `gc` consecutive segments of the flattened (row, segment) index q = b m + p, starting at q0; sequence q nch + channel.
struct WelchGen {
    const void *x, *y, *win;
    void *seg;  // [gc nch][n] T
    unsigned long long sample_stride, q0, gc, m;
    unsigned n, hop, nch;
    int detrend;
    double inv_n, inv_sxx;
};

template <typename T>
__device__ __forceinline__ T block_sum(T v, T *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (unsigned w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// one workgroup per sequence: the detrended, windowed segment
template <typename T>
__global__ __launch_bounds__(256) void k_welch_gather(WelchGen g) {
    __shared__ T sh[256];
    for (unsigned long long sq = blockIdx.x; sq < g.gc * g.nch; sq += gridDim.x) {  // (uniform per workgroup)
        const unsigned long long q = g.q0 + sq / g.nch, b = q / g.m, p = q % g.m;
        const T *src = (const T *)((sq % g.nch) ? g.y : g.x) + b * g.sample_stride + p * g.hop;
        const T *win = (const T *)g.win;
        T *dst = (T *)g.seg + sq * g.n;
        const T ctr = T(0.5 * double(g.n - 1));
        // the mean in two steps and the slope fitted to the remainders, as k_welch does (the reasons are there)
        T mu = T(0), mu2 = T(0), slope = T(0);
        if (g.detrend != SGX_WELCH_DETREND_NONE) {
            T s0 = T(0);
            for (unsigned j = threadIdx.x; j < g.n; j += 256) s0 += src[j];
            mu = block_sum(s0, sh) * T(g.inv_n);
            s0 = T(0);
            for (unsigned j = threadIdx.x; j < g.n; j += 256) s0 += src[j] - mu;
            mu2 = block_sum(s0, sh) * T(g.inv_n);
            if (g.detrend == SGX_WELCH_DETREND_LINEAR) {
                T s1 = T(0);
                for (unsigned j = threadIdx.x; j < g.n; j += 256) s1 += (T(j) - ctr) * ((src[j] - mu) - mu2);
                slope = block_sum(s1, sh) * T(g.inv_sxx);
            }
        }
        for (unsigned j = threadIdx.x; j < g.n; j += 256) dst[j] = (((src[j] - mu) - mu2) - slope * (T(j) - ctr)) * win[j];
    }
}

// acc [batch][nacc][nb] += the chunk's segments, a row's segments in order
template <typename T, int KIND>
__global__ __launch_bounds__(256) void k_welch_accum(const typename PairOf<T>::type *spec, T *acc, unsigned long long q0, unsigned long long gc,
                                                     unsigned long long m, unsigned nb, unsigned long long b_lo, unsigned long long total) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned NCH = KIND == KIND_PSD ? 1 : 2, NACC = welch_nacc(KIND);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long b = b_lo + i / nb;
        const unsigned k = (unsigned)(i % nb);
        const unsigned long long lo = b * m > q0 ? b * m : q0, hi = (b + 1) * m < q0 + gc ? (b + 1) * m : q0 + gc;
        T *dst = acc + b * NACC * nb + k;
        T s[NACC];
#pragma unroll
        for (unsigned c = 0; c < NACC; ++c) s[c] = dst[(size_t)c * nb];
        for (unsigned long long q = lo; q < hi; ++q) {
            const V X = spec[((q - q0) * NCH) * nb + k];
            const V Y = NCH > 1 ? spec[((q - q0) * NCH + 1) * nb + k] : X;
            welch_add<KIND, T, V>(s, 1, X, Y);
        }
#pragma unroll
        for (unsigned c = 0; c < NACC; ++c) dst[(size_t)c * nb] = s[c];
    }
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_welch {
    size_t n = 0, hop = 0, nb = 0;
    int kind = KIND_PSD, detrend = SGX_WELCH_DETREND_CONSTANT, scaling = SGX_WELCH_DENSITY;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4, max_scratch = kDefaultScratch;
    double sample_rate = 1.0, scale = 0.0;
    bool fused = false;
    unsigned fa = 0, fb = 0, fc = 0, tile = 0, sub = 0;
    std::vector<double> window;
    DevBuf d_win, d_tw;
    PlanHandle fft;  // generic route: one frame of n samples per row
    DevBuf d_part, d_seg, d_spec, d_in, d_in2, d_out;
    size_t allocations = 0;
    mutable std::string err;
};

namespace {

unsigned nacc_of(const sgx_welch *p) { return welch_nacc(p->kind); }
unsigned nch_of(const sgx_welch *p) { return p->kind == KIND_PSD ? 1u : 2u; }

sgx_status wgrow(sgx_welch *p, DevBuf &b, size_t need) {
    if (b.bytes >= need) return SGX_OK;
    ++p->allocations;
    return grow(p, b, need);
}

size_t fused_seq_bytes(const sgx_welch *p) {
    return rr_seq_bytes(2 * (unsigned)p->elem, p->fa, p->fb, p->fc);
}

template <typename T, int A, int B, int C, int KIND>
hipError_t launch_welch_t(const WelchArgs &a, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024) {
        const hipError_t e = set_max_dynamic_lds((const void *)k_welch<T, A, B, C, KIND>, (int)kWelchLdsMax);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_welch<T, A, B, C, KIND>), dim3(xcd_grid((unsigned long long)a.tiles * a.batch)), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <typename T, int A, int B, int C>
hipError_t launch_welch_k(int kind, const WelchArgs &a, size_t lds, hipStream_t s) {
    if (kind == KIND_PSD) return launch_welch_t<T, A, B, C, KIND_PSD>(a, lds, s);
    if (kind == KIND_CSD) return launch_welch_t<T, A, B, C, KIND_CSD>(a, lds, s);
    return launch_welch_t<T, A, B, C, KIND_COH>(a, lds, s);
}

// the (A, B, C) splits reg_split_len gives the powers of two 256 .. 4096 (as k_fir_os)
#define SGX_WELCH_SPLITS_F32(X) X(16, 16, 1) X(8, 8, 8) X(16, 8, 8) X(16, 16, 8) X(16, 16, 16)
#define SGX_WELCH_SPLITS_F64(X) X(8, 8, 4) X(8, 8, 8) X(16, 8, 8) X(16, 16, 8) X(16, 16, 16)

bool fused_split_known(int dtype, unsigned fa, unsigned fb, unsigned fc) {
    return dtype == SGX_F64 ? SGX_RR_SPLIT_IN(SGX_WELCH_SPLITS_F64, fa, fb, fc) : SGX_RR_SPLIT_IN(SGX_WELCH_SPLITS_F32, fa, fb, fc);
}

hipError_t launch_fused(const sgx_welch *p, const WelchArgs &a, hipStream_t s) {
    // sums behind the rounds reuse the sequences' LDS: [NBK <= 9][256] T fits below one sequence of every split
    const size_t lds = (size_t)p->sub * nch_of(p) * fused_seq_bytes(p);
    const unsigned fa = p->fa, fb = p->fb, fc = p->fc;
#define SGX_WELCH_F32(A, B, C) if (fa == A && fb == B && fc == C) return launch_welch_k<float, A, B, C>(p->kind, a, lds, s);
#define SGX_WELCH_F64(A, B, C) if (fa == A && fb == B && fc == C) return launch_welch_k<double, A, B, C>(p->kind, a, lds, s);
    if (p->dtype == SGX_F64) { SGX_WELCH_SPLITS_F64(SGX_WELCH_F64) } else { SGX_WELCH_SPLITS_F32(SGX_WELCH_F32) }
#undef SGX_WELCH_F32
#undef SGX_WELCH_F64
    return hipErrorNotSupported;
}

size_t segments_of(const sgx_welch *p, size_t n_samples) { return n_samples < p->n ? 0 : 1 + (n_samples - p->n) / p->hop; }
size_t tiles_of(const sgx_welch *p, size_t m) { return p->fused ? (m + p->tile - 1) / p->tile : 1; }

// generic route: segments per chunk (a segment's sequences: nch real rows of n, nch half spectra of nb complex bins)
size_t gen_chunk(const sgx_welch *p, size_t total) {
    const size_t per = nch_of(p) * std::max(p->n, 2 * p->nb) * p->elem;
    return std::max<size_t>(1, std::min(total, p->max_scratch / per));
}

sgx_status reserve_dev(sgx_welch *p, size_t batch, size_t m) {
    sgx_status st;
    if ((st = wgrow(p, p->d_part, batch * tiles_of(p, m) * nacc_of(p) * p->nb * p->elem)) != SGX_OK) return st;
    if (!p->fused) {
        const size_t gc = gen_chunk(p, batch * m), rows = gc * nch_of(p);
        if ((st = wgrow(p, p->d_seg, rows * p->n * p->elem)) != SGX_OK) return st;
        if ((st = wgrow(p, p->d_spec, rows * p->nb * 2 * p->elem)) != SGX_OK) return st;
        if (sgx_reserve(p->fft.get(), rows, p->n, 0, 0) != SGX_OK) return fail(p, SGX_BACKEND, sgx_last_error(p->fft.get()));
    }
    return SGX_OK;
}

template <typename T>
hipError_t launch_fold(const sgx_welch *p, void *out, size_t batch, size_t m, hipStream_t s) {
    const unsigned long long total = (unsigned long long)batch * p->nb;
    hipLaunchKernelGGL(k_welch_fold<T>, dim3(grid_for_items(total)), dim3(256), 0, s, p->d_part.as<T>(), (T *)out, unsigned(p->nb),
                       unsigned(tiles_of(p, m)), unsigned(p->n), p->kind, p->scale / double(m), total);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_accum(const sgx_welch *p, unsigned long long q0, unsigned long long gc, unsigned long long m, hipStream_t s) {
    typedef typename PairOf<T>::type V;
    const unsigned long long b_lo = q0 / m, b_hi = (q0 + gc - 1) / m, total = (b_hi - b_lo + 1) * p->nb;
    const dim3 grid(grid_for_items(total));
    if (p->kind == KIND_PSD)
        hipLaunchKernelGGL((k_welch_accum<T, KIND_PSD>), grid, dim3(256), 0, s, p->d_spec.as<V>(), p->d_part.as<T>(), q0, gc, m, unsigned(p->nb), b_lo, total);
    else if (p->kind == KIND_CSD)
        hipLaunchKernelGGL((k_welch_accum<T, KIND_CSD>), grid, dim3(256), 0, s, p->d_spec.as<V>(), p->d_part.as<T>(), q0, gc, m, unsigned(p->nb), b_lo, total);
    else
        hipLaunchKernelGGL((k_welch_accum<T, KIND_COH>), grid, dim3(256), 0, s, p->d_spec.as<V>(), p->d_part.as<T>(), q0, gc, m, unsigned(p->nb), b_lo, total);
    return hipGetLastError();
}

sgx_status run_dev(sgx_welch *p, const void *x, const void *y, size_t batch, size_t n_samples, size_t stride, void *out, hipStream_t s) {
    const size_t m = segments_of(p, n_samples);
    sgx_status st = reserve_dev(p, batch, m);
    if (st != SGX_OK) return st;
    const double nn = double(p->n);
    const double inv_n = 1.0 / nn, inv_sxx = p->n > 1 ? 12.0 / (nn * (nn * nn - 1.0)) : 0.0;
    const bool f64 = p->dtype == SGX_F64;
    if (p->fused) {
        WelchArgs a{};
        a.x = x; a.y = y; a.part = p->d_part; a.win = p->d_win; a.tw = p->d_tw;
        a.sample_stride = stride;
        a.batch = unsigned(batch); a.hop = unsigned(p->hop); a.nseg = unsigned(m);
        a.tile = p->tile; a.sub = p->sub; a.tiles = unsigned(tiles_of(p, m));
        a.detrend = p->detrend; a.inv_n = inv_n; a.inv_sxx = inv_sxx;
        SGX_TRY_HIP(p, launch_fused(p, a, s));
    } else {
        const size_t total = batch * m, gc = gen_chunk(p, total);
        const unsigned nch = nch_of(p);
        SGX_TRY_HIP(p, hipMemsetAsync(p->d_part, 0, batch * nacc_of(p) * p->nb * p->elem, s));
        WelchGen g{};
        g.x = x; g.y = y; g.win = p->d_win; g.seg = p->d_seg;
        g.sample_stride = stride; g.m = m; g.n = unsigned(p->n); g.hop = unsigned(p->hop); g.nch = nch;
        g.detrend = p->detrend; g.inv_n = inv_n; g.inv_sxx = inv_sxx;
        sgx_plan *fft = p->fft.get();
        for (size_t q0 = 0; q0 < total; q0 += gc) {
            g.q0 = q0;
            g.gc = std::min(gc, total - q0);
            const size_t rows = g.gc * nch;
            const unsigned grid = unsigned(std::min<size_t>(rows, size_t(1) << 20));
            if (f64) hipLaunchKernelGGL(k_welch_gather<double>, dim3(grid), dim3(256), 0, s, g);
            else hipLaunchKernelGGL(k_welch_gather<float>, dim3(grid), dim3(256), 0, s, g);
            SGX_TRY_HIP(p, hipGetLastError());
            if (sgx_execute(fft, p->d_seg, rows, p->n, p->n, p->d_spec, rows * p->nb * 2, SGX_MEM_DEVICE, s) != SGX_OK)
                return fail(p, SGX_BACKEND, sgx_last_error(fft));
            SGX_TRY_HIP(p, f64 ? launch_accum<double>(p, q0, g.gc, m, s) : launch_accum<float>(p, q0, g.gc, m, s));
        }
    }
    SGX_TRY_HIP(p, f64 ? launch_fold<double>(p, out, batch, m, s) : launch_fold<float>(p, out, batch, m, s));
    return SGX_OK;
}

}  // namespace

extern "C" {

sgx_status sgx_welch_create(const sgx_params *params, int32_t kind, int32_t detrend, int32_t scaling, int32_t route, size_t max_scratch_bytes,
                            sgx_welch **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_welch>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out || !params) return bad("null argument");
    if (kind != KIND_PSD && kind != KIND_CSD && kind != KIND_COH) return bad("unknown kind (PSD, CSD or coherence)");
    if (detrend != SGX_WELCH_DETREND_NONE && detrend != SGX_WELCH_DETREND_CONSTANT && detrend != SGX_WELCH_DETREND_LINEAR)
        return bad("unknown detrend (none, constant or linear)");
    if (scaling != SGX_WELCH_DENSITY && scaling != SGX_WELCH_SPECTRUM) return bad("unknown scaling (density or spectrum)");
    if (route != SGX_WELCH_ROUTE_AUTO && route != SGX_WELCH_ROUTE_GENERIC) return bad("unknown route");
    if (params->centre) return bad("centre must be 0 for a Welch plan (segments are not padded)");
    if (params->dtype != SGX_F32 && params->dtype != SGX_F64) return bad("dtype must be f32 or f64");
    // every STFT check of sgx_plan_create (n_fft, hop_size, the window and its parameter, the sample rate), and the window as it builds it
    sgx_params sp{};
    sp.n_fft = params->n_fft; sp.hop_size = params->hop_size; sp.centre = 0;
    sp.window_kind = params->window_kind; sp.window_param = params->window_param;
    sp.custom_window = params->custom_window; sp.custom_window_len = params->custom_window_len;
    sp.sample_rate_hz = params->sample_rate_hz;
    sp.freq_scale = SGX_FREQ_LINEAR; sp.amp_scale = SGX_AMP_COMPLEX;
    sp.dtype = params->dtype; sp.device = -2;
    PlanHandle host;
    {
        sgx_plan *raw = nullptr;
        const sgx_status st = sgx_plan_create(&sp, &raw);
        host.reset(raw);
        if (st != SGX_OK) return fail<sgx_welch>(nullptr, st, sgx_last_create_error());
    }
    sgx_welch *p = new (std::nothrow) sgx_welch();
    if (!p) return fail<sgx_welch>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->n = params->n_fft; p->hop = params->hop_size; p->nb = p->n / 2 + 1;
    p->kind = kind; p->detrend = detrend; p->scaling = scaling;
    p->dtype = params->dtype; p->elem = elem_size(p->dtype); p->device = params->device;
    p->sample_rate = params->sample_rate_hz;
    p->max_scratch = max_scratch_bytes ? max_scratch_bytes : kDefaultScratch;
    p->window.resize(p->n);
    (void)sgx_window(host.get(), p->window.data());
    host.reset();
    // sums in extended precision, the factor rounded once: a plain f64 running sum over 4096 coefficients is off by 20 u, which an
    // f64 plan would carry into every bin as a common factor (measured: 42 u on the "spectrum" scale at n_fft 4096)
    long double sw = 0.0L, sw2 = 0.0L;
    for (double w : p->window) { sw += (long double)w; sw2 += (long double)w * (long double)w; }
    p->scale = double(scaling == SGX_WELCH_DENSITY ? 1.0L / ((long double)p->sample_rate * sw2) : 1.0L / (sw * sw));
    const unsigned n = unsigned(p->n);
    p->fused = route == SGX_WELCH_ROUTE_AUTO && n >= 256 && n <= 4096 && (n & (n - 1)) == 0 &&
               reg_split_len(n, p->dtype, &p->fa, &p->fb, &p->fc) && fused_split_known(p->dtype, p->fa, p->fb, p->fc) &&
               2 * fused_seq_bytes(p) <= kWelchLdsMax;
    if (p->fused) {
        // a round holds `sub` segments (a PSD plan takes the pair kinds' count: the same segments meet in the same sums, so that
        // csd(x, x) is welch(x) bit for bit); a tile is whole rounds, about 8 n samples of new input, at most kWelchMaxTile segments
        const size_t per = 2 * fused_seq_bytes(p);
        unsigned sub = 16;
        while (sub > 1 && sub * per > kWelchLdsRound) sub >>= 1;
        p->sub = sub;
        const size_t want = (8 * p->n + p->hop - 1) / p->hop;
        p->tile = unsigned(std::min<size_t>(kWelchMaxTile, std::max<size_t>(sub, (want + sub - 1) / sub * sub)));
    }
    auto tables = [&]() -> sgx_status {
        if (!p->fused) {  // (a host-only plan keeps a host-only transform: its checks of n_fft are the route's)
            const sgx_status st = create_row_fft(p->n, p->dtype, p->device, p->fft);
            if (st != SGX_OK) return fail(p, st, sgx_last_create_error());
            if (p->device != -2) p->device = sgx_plan_device(p->fft.get());
        }
        if (p->device == -2) return SGX_OK;
        if (p->device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        sgx_status st;
        if ((st = upload(p, p->d_win, p->window, p->dtype)) != SGX_OK) return st;
        if (p->fused) {
            // W_n^k rounded once from extended precision: the f64 argument 2 pi k / n alone is off by up to 2 pi u, which the f64 kernels
            // would carry into every bin (measured: 2.7 times the f32 kernels' error in units of u)
            std::vector<double> tw(2 * p->n);
            const long double two_pi = 6.283185307179586476925286766559005768L;
            for (size_t k = 0; k < p->n; ++k) {
                const long double a = -two_pi * (long double)k / (long double)p->n;
                tw[2 * k] = double(std::cos(a));
                tw[2 * k + 1] = double(std::sin(a));
            }
            if ((st = upload(p, p->d_tw, tw, p->dtype)) != SGX_OK) return st;
        }
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_welch_destroy);
}

void sgx_welch_destroy(sgx_welch *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device >= 0) (void)dg.enter(p->device);
    delete p;
}

size_t sgx_welch_n_bins(const sgx_welch *p) { return p ? p->nb : 0; }
size_t sgx_welch_n_segments(const sgx_welch *p, size_t n_samples) { return p ? segments_of(p, n_samples) : 0; }

sgx_status sgx_welch_frequencies(const sgx_welch *p, double *freqs) {
    if (!p || !freqs) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    const double d = 1.0 / p->sample_rate, val = 1.0 / (double(p->n) * d);  // (numpy.fft.rfftfreq's two steps)
    for (size_t k = 0; k < p->nb; ++k) freqs[k] = double(k) * val;
    return SGX_OK;
}

sgx_status sgx_welch_window(const sgx_welch *p, double *window) {
    if (!p || !window) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->window.begin(), p->window.end(), window);
    return SGX_OK;
}

double sgx_welch_scale(const sgx_welch *p) { return p ? p->scale : 0.0; }

sgx_status sgx_welch_reserve(sgx_welch *p, size_t batch, size_t n_samples, int32_t host_staging) {
    if (!p || batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (n_samples < p->n) return dim_mismatch(p, p->n, n_samples, " (n_samples must be at least n_fft)");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    if ((st = reserve_dev(p, batch, segments_of(p, n_samples))) != SGX_OK) return st;
    if (host_staging) {
        if ((st = wgrow(p, p->d_in, batch * n_samples * p->elem)) != SGX_OK) return st;
        if (nch_of(p) > 1 && (st = wgrow(p, p->d_in2, batch * n_samples * p->elem)) != SGX_OK) return st;
        if ((st = wgrow(p, p->d_out, batch * p->nb * (p->kind == KIND_CSD ? 2 : 1) * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_welch_execute(sgx_welch *p, const void *x, const void *y, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                             size_t out_elems, int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!x || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (p->kind == KIND_PSD && y) return fail(p, SGX_INVALID_INPUT, "Invalid input: y must be NULL for a PSD plan");
    if (p->kind != KIND_PSD && !y) return fail(p, SGX_INVALID_INPUT, "Invalid input: y is required by a CSD / coherence plan");
    if (batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (n_samples < p->n) return dim_mismatch(p, p->n, n_samples, " (n_samples must be at least n_fft)");
    if (sample_stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    const size_t per_row = p->nb * (p->kind == KIND_CSD ? 2 : 1);
    if (out_elems != batch * per_row) return dim_mismatch(p, batch * per_row, out_elems);
    const size_t m = segments_of(p, n_samples);
    if (batch > 0xffffffffull || n_samples > (size_t(1) << 40) || m >= 0x7fffffffull || tiles_of(p, m) * batch >= 0x7fffffffull)
        return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return run_dev(p, x, y, batch, n_samples, sample_stride, out, s);
    const size_t in_bytes = ((batch - 1) * sample_stride + n_samples) * p->elem, out_bytes = out_elems * p->elem;
    sgx_status st;
    if ((st = wgrow(p, p->d_in, in_bytes)) != SGX_OK) return st;
    if (y && (st = wgrow(p, p->d_in2, in_bytes)) != SGX_OK) return st;
    if ((st = wgrow(p, p->d_out, out_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
    if (y) SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in2, y, in_bytes, hipMemcpyHostToDevice, s));
    if ((st = run_dev(p, p->d_in, y ? p->d_in2.ptr : nullptr, batch, n_samples, sample_stride, p->d_out, s)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

size_t sgx_welch_allocations(const sgx_welch *p) { return p ? p->allocations : 0; }
size_t sgx_welch_tile(const sgx_welch *p) { return p && p->fused ? p->tile : 0; }
const char *sgx_welch_kernel_name(const sgx_welch *p) { return !p ? "" : p->fused ? "k_welch" : "welch_generic"; }
int32_t sgx_welch_device(const sgx_welch *p) { return p ? p->device : -2; }
const char *sgx_welch_last_error(const sgx_welch *p) { return p ? p->err.c_str() : create_err<sgx_welch>().c_str(); }

}  // extern "C"

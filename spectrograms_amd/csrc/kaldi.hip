// kaldi.hip — batched Kaldi-compatible filterbank / MFCC features (sgx_kaldi_*) of libspectro_hip.so, kernels and host side.
//
// Semantics (torchaudio.compliance.kaldi.fbank / .mfcc with dither = 0 and vtln_warp = 1, one row per batch item): frames of
// N = int(fs frame_length_ms / 1000) samples every shift = int(fs frame_shift_ms / 1000), zero-padded to P (the next power of two, or N);
// snip_edges: m = 1 + (n - N) / shift frames from t shift; otherwise m = (n + shift / 2) / shift frames from t shift + shift / 2 - N / 2
// with the row mirrored at both ends (index i < 0 reads x[-i - 1], i >= n reads x[2 n - 1 - i]).  Per frame, in this order: subtract the
// frame's mean; the raw log energy; f[j] - alpha f[j - 1] with f[-1] := f[0]; the window; the log energy if not raw; the real FFT of P
// points; |X| or |X|^2; E = spectrum . bank^T; log(max(E, eps_T)); for MFCC the first num_ceps rows of the orthonormal DCT-II and the
// lifter; the energy column; the column means over the row's frames (subtract_mean).  Output [batch][m][n_out] T.
// A maximum is one that keeps a NaN (v < lo ? lo : v): a frame that holds a non-finite sample is non-finite in every feature, as torch.max
// leaves it, and no other frame is.
//
// Routes:
//   k_kaldi<T, A, B, C>    P = A B C in 256 .. 2048 (the splits of k_fir_os / k_welch).  A workgroup takes a tile of `tile` consecutive
//                          frames of one row, `sub` of them per round through LDS.  Pass 1 loads a frame's samples (and each sample's
//                          predecessor, which sits in the same cache lines) into its work items' registers, forms the mean across the
//                          work items that hold the frame in two steps as k_welch does (welch.hip:14 has the reason the mean leaves the
//                          samples before anything else is done to them), the energy, the pre-emphasis difference and the window
//                          product; points N .. P - 1 are zero.  The passes of the complex transform run on the real sequence.  The
//                          last pass writes |X|^2 or |X| of bins 0 .. P / 2 - 1 to LDS (the bank's Nyquist column is zero); one work
//                          item per (frame, band) adds its CSR row (from the workgroup's LDS copy of the bank) in ascending bin order
//                          and takes the log; one work item per (frame, column) runs the DCT's fma chain over the bands in ascending
//                          order and stores; a frame's n_out values are contiguous.  Blocks are ordered with xcd_map.h (neighbouring
//                          frames share most of their samples).
//   kaldi_generic          every other P an sgx_plan transforms, and any P when asked for: k_kaldi_gather writes the preprocessed,
//                          padded frames of a chunk to scratch, an internal one-frame-per-row plan (create_row_fft) transforms them,
//                          k_kaldi_bank does bank, log, DCT and energy; chunks of at most max_scratch_bytes per buffer.  A frame's bits
//                          depend on its own samples alone, so the chunk seams do not change them.
// k_kaldi_cmn (subtract_mean) adds a row's frames per column in frame order and subtracts in place.  No atomics anywhere: a row's bits
// depend on nothing but its own samples.
// The tables (window, bank, DCT, lifter) are built in extended precision on the host and rounded once to f64, then cast to T; torchaudio
// builds them in f32.
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

constexpr size_t kKaldiLdsRound = 48 * 1024;  // LDS of one round: the frames' sequences, spectra, band logs and energies
constexpr size_t kKaldiLdsMax = 64 * 1024;    // ... and of the workgroup with its copy of the bank; one frame always fits
constexpr unsigned kKaldiTile = 32;           // frames per workgroup (whole rounds: sub divides it)
constexpr unsigned kKaldiMaxFusedBins = 256;  // bands whose logs a round keeps in LDS
constexpr unsigned kKaldiMaxBins = 8192;      // k_kaldi_bank keeps one frame's band logs in LDS
constexpr size_t kDefaultScratch = size_t(256) << 20;

struct KaldiArgs {
    const void *x;          // [batch][sample_stride] T
    void *out;              // [batch][m][n_out] T
    const void *win;        // [N] T
    const void *tw;         // [P] complex T: W_P^k (fused route)
    const unsigned *band;   // [bins][3]: first bin, bins, offset into bval
    const void *bval;       // the bank's positive weights, band after band
    const void *dct;        // [num_ceps][bins] T
    const void *lifter;     // [num_ceps] T
    unsigned long long sample_stride, n_samples, m;
    unsigned batch, N, shift, tiles, tile, sub, bins, num_ceps, n_out, nval;
    int snip_edges, remove_dc, raw_energy, use_energy, use_power, use_log, htk_compat, has_floor, preemph;
    double alpha, eps, log_floor;
};

// a maximum that keeps a NaN in v
template <typename T>
__device__ __forceinline__ T nan_max(T v, T lo) { return v < lo ? lo : v; }

__device__ __forceinline__ float k_log(float v) { return logf(v); }
__device__ __forceinline__ double k_log(double v) { return log(v); }
__device__ __forceinline__ float k_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double k_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float k_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double k_fma(double a, double b, double c) { return fma(a, b, c); }

// sample i of the frame space: mirrored at both ends without snip_edges; every index ends inside the row
template <typename T>
__device__ __forceinline__ T kaldi_sample(const T *x, long long i, long long n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    i = i < 0 ? 0 : (i >= n ? n - 1 : i);
    return x[i];
}

__device__ __forceinline__ long long kaldi_frame_start(const KaldiArgs &a, unsigned long long t) {
    const long long s = (long long)(t * a.shift);
    return a.snip_edges ? s : s + (long long)(a.shift / 2) - (long long)(a.N / 2);
}

template <typename T>
__device__ __forceinline__ T kaldi_log_energy(const KaldiArgs &a, T sum) {
    T e = k_log(nan_max(sum, T(a.eps)));
    if (a.has_floor) e = nan_max(e, T(a.log_floor));
    return e;
}

// acc + sum_i w[i] v[i] as one fma chain in ascending order; the operands of four links are fetched together, ahead of the chain
template <typename T>
__device__ __forceinline__ T kaldi_chain(const T *w, const T *v, unsigned cnt, T acc) {
    unsigned i = 0;
    for (; i + 4 <= cnt; i += 4) {
        const T w0 = w[i], w1 = w[i + 1], w2 = w[i + 2], w3 = w[i + 3];
        const T v0 = v[i], v1 = v[i + 1], v2 = v[i + 2], v3 = v[i + 3];
        acc = k_fma(w3, v3, k_fma(w2, v2, k_fma(w1, v1, k_fma(w0, v0, acc))));
    }
    for (; i < cnt; ++i) acc = k_fma(w[i], v[i], acc);
    return acc;
}

// band b of one frame: the CSR row's products added in ascending bin order, then the log (band, bval: the plan's tables or a copy)
template <typename T>
__device__ __forceinline__ T kaldi_band(const KaldiArgs &a, const unsigned *band, const T *bval, unsigned b, const T *spec) {
    const unsigned lo = band[3 * b], cnt = band[3 * b + 1], off = band[3 * b + 2];
    const T e = kaldi_chain(bval + off, spec + lo, cnt, T(0));
    return a.use_log ? k_log(nan_max(e, T(a.eps))) : e;
}

// column c of one frame's features from its band values L and its log energy
template <typename T>
__device__ __forceinline__ T kaldi_column(const KaldiArgs &a, unsigned c, const T *L, T energy) {
    if (a.num_ceps == 0) {
        if (a.use_energy) {
            if (a.htk_compat) {
                if (c == a.bins) return energy;
            } else {
                if (c == 0) return energy;
                c -= 1;
            }
        }
        return L[c];
    }
    const unsigned i = a.htk_compat ? (c + 1 == a.num_ceps ? 0u : c + 1) : c;
    if (i == 0 && a.use_energy) return energy;
    return kaldi_chain((const T *)a.dct + (size_t)i * a.bins, L, a.bins, T(0)) * ((const T *)a.lifter)[i];
}

template <typename T, int A_, int B_, int C_>
__global__ __launch_bounds__(256, (rr_waves<T, A_, B_, C_>())) void k_kaldi(KaldiArgs a) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, B = B_, C = C_, BC = B * C, P = A * BC, HP = P / 2;
    constexpr unsigned LAST = C > 1 ? C : B;
    constexpr unsigned Q = C > 1 ? A * B : A;                 // work items of the last pass per frame
    constexpr unsigned W = BC < 64 ? BC : 64, WPS = BC / W;   // lanes of a wave, waves, that hold one frame in pass 1
    constexpr bool kTableTwiddles = sizeof(T) == 8;           // f64: every twiddle read from the table (f32 builds them from LA entries)
    static_assert(ct_is_pow2(P) && 256 % Q == 0 && 256 % BC == 0 && WPS <= 4, "k_kaldi: power-of-two splits of k_fir_os");
    typedef RrLayout<sizeof(V), A_, B_, C_> Lay;
    constexpr unsigned FS = Lay::FS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ T red[2][3][4];  // pass 1, frames over several waves: the waves' sums, one slot per reduction, two iterations' worth
    V *buf = (V *)smem;                      // [sub][FS]
    T *spec = (T *)(buf + (size_t)a.sub * FS);  // [sub][HP]
    T *Lb = spec + (size_t)a.sub * HP;          // [sub][bins]
    T *en = Lb + (size_t)a.sub * a.bins;        // [sub]
    T *bw = en + a.sub;                         // [nval]: the bank's weights ...
    unsigned *bd = (unsigned *)(bw + a.nval);   // [bins][3]: ... and its rows, read by every round
    const unsigned tid = threadIdx.x;
    const unsigned lb = xcd_logical_block(a.tiles * a.batch);  // neighbouring tiles share sample lines: keep them in one XCD
    if (lb >= a.tiles * a.batch) return;
    const unsigned t = lb % a.tiles, b = lb / a.tiles;
    const unsigned p0 = t * a.tile, nf = (unsigned)min((unsigned long long)a.tile, a.m - p0);
    const T *x = (const T *)a.x + (size_t)b * a.sample_stride;
    T *out = (T *)a.out + ((size_t)b * a.m + p0) * a.n_out;
    const T *win = (const T *)a.win;
    const V *tw = (const V *)a.tw;
    const T alpha = T(a.alpha), cnt = T(a.N);
    const long long n = (long long)a.n_samples;
    for (unsigned i = tid; i < a.nval; i += 256) bw[i] = ((const T *)a.bval)[i];
    for (unsigned i = tid; i < 3 * a.bins; i += 256) bd[i] = a.band[i];  // (read behind the barriers of the first round)

    unsigned round = 0;
    for (unsigned s0 = 0; s0 < nf; s0 += a.sub) {
        const unsigned nq = min(a.sub, nf - s0);  // frames of this round
        // P1 + T1: z[j] = w[j] (f[j] - alpha f[j - 1]), f = x_t - mean, for j = n1 B C + r < N; zero from N on
        const unsigned items = nq * BC, iters = (items + 255u) / 256u;
        for (unsigned it = 0; it < iters; ++it, ++round) {
            const unsigned idx = tid + 256u * it, sq = idx / BC, r = idx % BC;
            const bool valid = idx < items;
            T xv[A], xp[A];
#pragma unroll
            for (unsigned n1 = 0; n1 < A; ++n1) xv[n1] = xp[n1] = T(0);
            if (valid) {
                const long long f0 = kaldi_frame_start(a, (unsigned long long)p0 + s0 + sq);
                if (f0 >= 0 && f0 + (long long)a.N <= n) {  // (uniform per frame) a frame inside the row: no index is mirrored
                    const T *pf = x + f0;
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) {
                        const unsigned j = n1 * BC + r;
                        if (j < a.N) {
                            xv[n1] = pf[j];
                            if (a.preemph) xp[n1] = pf[j ? j - 1 : 0];
                        }
                    }
                } else {
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) {
                        const unsigned j = n1 * BC + r;
                        if (j < a.N) {
                            xv[n1] = kaldi_sample(x, f0 + j, n);
                            if (a.preemph) xp[n1] = kaldi_sample(x, f0 + (j ? j - 1 : 0), n);
                        }
                    }
                }
            }
            // The sum of a value over the work items of the frame (reduction `slot` of this iteration; every work item ends with the
            // same bits).  A slot's words are rewritten two iterations later, behind the barrier of the iteration between.
            auto seq_sum = [&](T v, unsigned slot) {
#pragma unroll
                for (unsigned off = 1; off < W; off <<= 1) v += __shfl_xor(v, off, 64);
                if constexpr (WPS > 1) {
                    T(*rd)[4] = red[round & 1u];
                    const unsigned wv = tid >> 6, w0 = wv / WPS * WPS;
                    if ((tid & 63u) == 0) rd[slot][wv] = v;
                    __syncthreads();
                    v = rd[slot][w0];
#pragma unroll
                    for (unsigned j = 1; j < WPS; ++j) v += rd[slot][w0 + j];
                }
                return v;
            };
            if (a.remove_dc) {  // (uniform) the mean in two steps, as k_welch: the mean of the remainders takes the first one's rounding
#pragma unroll
                for (unsigned pass = 0; pass < 2; ++pass) {
                    T s = T(0);
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) s += xv[n1];
                    const T mu = seq_sum(s, pass) / cnt;
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1)
                        if (n1 * BC + r < a.N) {
                            xv[n1] -= mu;
                            xp[n1] -= mu;
                        }
                }
            }
            T esum = T(0);
            if (a.use_energy && a.raw_energy) {  // (uniform)
#pragma unroll
                for (unsigned n1 = 0; n1 < A; ++n1) esum = k_fma(xv[n1], xv[n1], esum);
            }
            V v[A];
#pragma unroll
            for (unsigned n1 = 0; n1 < A; ++n1) {
                const unsigned j = n1 * BC + r;
                T z = T(0);
                if (j < a.N) {
                    z = a.preemph ? xv[n1] - alpha * xp[n1] : xv[n1];
                    z *= win[j];
                }
                v[n1] = (V){z, T(0)};
            }
            if (a.use_energy) {  // (uniform)
                if (!a.raw_energy) {
#pragma unroll
                    for (unsigned n1 = 0; n1 < A; ++n1) esum = k_fma(v[n1].x, v[n1].x, esum);
                }
                esum = seq_sum(esum, 2);
                if (valid && r == 0) en[sq] = kaldi_log_energy(a, esum);
            }
            if (!valid) continue;
            rr_pass1_store<T, A_, B_, C_, kTableTwiddles>(v, buf + (size_t)sq * FS, r, tw);
        }
        __syncthreads();
        if constexpr (C > 1) {
            // P2 + T2: this kernel's own copy of rr_pass2 (rr_passes.h).  With the shared loop, and with a per-item helper, the register
            // allocation of k_kaldi<float, 16, 16, 8> goes from 4 to 6 spilled registers (profiles/rr_passes_codegen.txt).
            constexpr unsigned RS = Lay::RS;
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
        // the last pass: work item q of a frame holds the bins k1 + A (k2 + B j) (three passes: q = k1 B + k2) or k1 + A j (two passes:
        // q = k1), j < LAST; those below P / 2 go to the frame's spectrum
        for (unsigned idx = tid; idx < nq * Q; idx += 256) {
            const unsigned s = idx / Q, q = idx % Q;
            const unsigned k1 = C > 1 ? q / B : q;
            const unsigned lp = (C > 1 ? Lay::hi_part(q % B) : 0u) ^ Lay::k1_mask(k1);
            V vx[LAST];
            rr_last_load<T, A_, B_, C_>(vx, buf + (size_t)s * FS + k1 * Lay::RS, lp);
            T *sp = spec + (size_t)s * HP;
#pragma unroll
            for (unsigned j = 0; j < LAST; ++j) {
                const unsigned k = C > 1 ? k1 + A * (q % B + B * j) : q + A * j;
                if (k < HP) {
                    const T pw = k_fma(vx[j].x, vx[j].x, vx[j].y * vx[j].y);
                    sp[k] = a.use_power ? pw : k_sqrt(pw);
                }
            }
        }
        __syncthreads();
        for (unsigned idx = tid; idx < nq * a.bins; idx += 256) {
            const unsigned s = idx / a.bins, bnd = idx % a.bins;
            Lb[idx] = kaldi_band<T>(a, bd, bw, bnd, spec + (size_t)s * HP);
        }
        __syncthreads();
        for (unsigned idx = tid; idx < nq * a.n_out; idx += 256) {
            const unsigned s = idx / a.n_out, c = idx % a.n_out;
            out[(size_t)s0 * a.n_out + idx] = kaldi_column(a, c, Lb + (size_t)s * a.bins, a.use_energy ? en[s] : T(0));
        }
        __syncthreads();  // the next round overwrites the energies and the spectra
    }
}

// ---- generic route ---------------------------------------------------------------------------------------------------------------
// A chunk is `gc` consecutive frames of the flattened (row, frame) index q = b m + t, starting at q0.
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

// one workgroup per frame: the preprocessed, windowed frame padded to P, and its log energy
template <typename T>
__global__ __launch_bounds__(256) void k_kaldi_gather(KaldiArgs a, T *seg, T *energy, unsigned long long q0, unsigned long long gc, unsigned P) {
    __shared__ T sh[256];
    const T *win = (const T *)a.win;
    const T alpha = T(a.alpha), cnt = T(a.N);
    const long long n = (long long)a.n_samples;
    for (unsigned long long sq = blockIdx.x; sq < gc; sq += gridDim.x) {  // (uniform per workgroup)
        const unsigned long long q = q0 + sq, b = q / a.m, t = q % a.m;
        const T *x = (const T *)a.x + b * a.sample_stride;
        const long long f0 = kaldi_frame_start(a, t);
        T *dst = seg + sq * P;
        T mu = T(0), mu2 = T(0);
        if (a.remove_dc) {  // the mean in two steps, as k_kaldi
            T s = T(0);
            for (unsigned j = threadIdx.x; j < a.N; j += 256) s += kaldi_sample(x, f0 + j, n);
            mu = block_sum(s, sh) / cnt;
            s = T(0);
            for (unsigned j = threadIdx.x; j < a.N; j += 256) s += kaldi_sample(x, f0 + j, n) - mu;
            mu2 = block_sum(s, sh) / cnt;
        }
        T esum = T(0);
        for (unsigned j = threadIdx.x; j < P; j += 256) {
            T z = T(0);
            if (j < a.N) {
                const T f = (kaldi_sample(x, f0 + j, n) - mu) - mu2;
                if (a.raw_energy) esum = k_fma(f, f, esum);
                z = f;
                if (a.preemph) z = f - alpha * ((kaldi_sample(x, f0 + (j ? j - 1 : 0), n) - mu) - mu2);
                z *= win[j];
                if (!a.raw_energy) esum = k_fma(z, z, esum);
            }
            dst[j] = z;
        }
        if (a.use_energy) {  // (uniform)
            esum = block_sum(esum, sh);
            if (threadIdx.x == 0) energy[sq] = kaldi_log_energy(a, esum);
        }
    }
}

// one workgroup per frame: bank, log, DCT and energy from the frame's half spectrum [P / 2 + 1] (the Nyquist bin is not read)
template <typename T>
__global__ __launch_bounds__(256) void k_kaldi_bank(KaldiArgs a, const typename PairOf<T>::type *spectra, const T *energy, unsigned long long q0,
                                                    unsigned long long gc, unsigned nb) {
    typedef typename PairOf<T>::type V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *L = (T *)smem;  // [bins]
    for (unsigned long long sq = blockIdx.x; sq < gc; sq += gridDim.x) {  // (uniform per workgroup)
        const V *sp = spectra + sq * nb;
        for (unsigned bnd = threadIdx.x; bnd < a.bins; bnd += 256) {
            const unsigned lo = a.band[3 * bnd], cnt = a.band[3 * bnd + 1], off = a.band[3 * bnd + 2];
            const T *w = (const T *)a.bval + off;
            T e = T(0);
            for (unsigned i = 0; i < cnt; ++i) {
                const V X = sp[lo + i];
                const T pw = k_fma(X.x, X.x, X.y * X.y);
                e = k_fma(w[i], a.use_power ? pw : k_sqrt(pw), e);
            }
            L[bnd] = a.use_log ? k_log(nan_max(e, T(a.eps))) : e;
        }
        __syncthreads();
        T *out = (T *)a.out + (q0 + sq) * a.n_out;  // (q = b m + t: the output's frame index)
        const T e = a.use_energy ? energy[sq] : T(0);
        for (unsigned c = threadIdx.x; c < a.n_out; c += 256) out[c] = kaldi_column(a, c, L, e);
        __syncthreads();
    }
}

// out[b][t][c] -= the mean over t, added in frame order
template <typename T>
__global__ __launch_bounds__(256) void k_kaldi_cmn(T *out, unsigned long long m, unsigned n_out, unsigned long long total) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        T *col = out + (i / n_out) * m * n_out + i % n_out;
        T s = T(0);
        for (unsigned long long t = 0; t < m; ++t) s += col[t * n_out];
        const T mu = s / T(m);
        for (unsigned long long t = 0; t < m; ++t) col[t * n_out] -= mu;
    }
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_kaldi {
    sgx_kaldi_params p{};
    size_t N = 0, shift = 0, P = 0, nb = 0, bins = 0, num_ceps = 0, n_out = 0;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4, max_scratch = kDefaultScratch;
    bool fused = false;
    unsigned fa = 0, fb = 0, fc = 0, tile = 0, sub = 0;
    size_t nval = 0;  // the bank's positive weights
    std::vector<double> window, bank, dct, lifter;  // [N], [bins][nb], [num_ceps][bins], [num_ceps]
    DevBuf d_win, d_tw, d_band, d_bval, d_dct, d_lifter;
    PlanHandle fft;  // generic route: one frame of P samples per row
    DevBuf d_seg, d_spec, d_energy, d_in, d_out;
    size_t allocations = 0;
    mutable std::string err;
};

namespace {

sgx_status kgrow(sgx_kaldi *p, DevBuf &b, size_t need) {
    if (b.bytes >= need) return SGX_OK;
    ++p->allocations;
    return grow(p, b, need);
}

size_t fused_frame_bytes(const sgx_kaldi *p) {
    const size_t seq = rr_seq_bytes(2 * (unsigned)p->elem, p->fa, p->fb, p->fc);
    return seq + (p->P / 2 + p->bins + 1) * p->elem;
}
// the workgroup's copy of the bank: its weights and its rows
size_t fused_bank_bytes(const sgx_kaldi *p) { return p->nval * p->elem + 3 * p->bins * sizeof(unsigned); }

template <typename T, int A, int B, int C>
hipError_t launch_kaldi_t(const KaldiArgs &a, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((k_kaldi<T, A, B, C>), dim3(xcd_grid((unsigned long long)a.tiles * a.batch)), dim3(256), lds, s, a);
    return hipGetLastError();
}

// the (A, B, C) splits reg_split_len gives the powers of two 256 .. 2048 (as k_fir_os and k_welch)
#define SGX_KALDI_SPLITS_F32(X) X(16, 16, 1) X(8, 8, 8) X(16, 8, 8) X(16, 16, 8)
#define SGX_KALDI_SPLITS_F64(X) X(8, 8, 4) X(8, 8, 8) X(16, 8, 8) X(16, 16, 8)

bool fused_split_known(int dtype, unsigned fa, unsigned fb, unsigned fc) {
    return dtype == SGX_F64 ? SGX_RR_SPLIT_IN(SGX_KALDI_SPLITS_F64, fa, fb, fc) : SGX_RR_SPLIT_IN(SGX_KALDI_SPLITS_F32, fa, fb, fc);
}

hipError_t launch_fused(const sgx_kaldi *p, const KaldiArgs &a, hipStream_t s) {
    const size_t lds = (size_t)p->sub * fused_frame_bytes(p) + fused_bank_bytes(p);
    const unsigned fa = p->fa, fb = p->fb, fc = p->fc;
#define SGX_KALDI_F32(A, B, C) if (fa == A && fb == B && fc == C) return launch_kaldi_t<float, A, B, C>(a, lds, s);
#define SGX_KALDI_F64(A, B, C) if (fa == A && fb == B && fc == C) return launch_kaldi_t<double, A, B, C>(a, lds, s);
    if (p->dtype == SGX_F64) { SGX_KALDI_SPLITS_F64(SGX_KALDI_F64) } else { SGX_KALDI_SPLITS_F32(SGX_KALDI_F32) }
#undef SGX_KALDI_F32
#undef SGX_KALDI_F64
    return hipErrorNotSupported;
}

size_t frames_of(const sgx_kaldi *p, size_t n) {
    if (n < p->N) return 0;
    return p->p.snip_edges ? 1 + (n - p->N) / p->shift : (n + p->shift / 2) / p->shift;
}

// generic route: frames per chunk (a frame: P reals, nb complex bins)
size_t gen_chunk(const sgx_kaldi *p, size_t total) {
    const size_t per = std::max(p->P, 2 * p->nb) * p->elem;
    return std::max<size_t>(1, std::min(total, p->max_scratch / per));
}

sgx_status reserve_dev(sgx_kaldi *p, size_t batch, size_t m) {
    if (p->fused) return SGX_OK;
    sgx_status st;
    const size_t gc = gen_chunk(p, batch * m);
    if ((st = kgrow(p, p->d_seg, gc * p->P * p->elem)) != SGX_OK) return st;
    if ((st = kgrow(p, p->d_spec, gc * p->nb * 2 * p->elem)) != SGX_OK) return st;
    if ((st = kgrow(p, p->d_energy, gc * p->elem)) != SGX_OK) return st;
    if (sgx_reserve(p->fft.get(), gc, p->P, 0, 0) != SGX_OK) return fail(p, SGX_BACKEND, sgx_last_error(p->fft.get()));
    return SGX_OK;
}

template <typename T>
hipError_t run_generic_chunk(sgx_kaldi *p, const KaldiArgs &a, size_t q0, size_t gc, int step, hipStream_t s) {
    typedef typename PairOf<T>::type V;
    const unsigned grid = unsigned(std::min<size_t>(gc, size_t(1) << 20));
    if (step == 0)
        hipLaunchKernelGGL(k_kaldi_gather<T>, dim3(grid), dim3(256), 0, s, a, p->d_seg.as<T>(), p->d_energy.as<T>(), (unsigned long long)q0,
                           (unsigned long long)gc, unsigned(p->P));
    else
        hipLaunchKernelGGL(k_kaldi_bank<T>, dim3(grid), dim3(256), p->bins * sizeof(T), s, a, p->d_spec.as<V>(), p->d_energy.as<T>(),
                           (unsigned long long)q0, (unsigned long long)gc, unsigned(p->nb));
    return hipGetLastError();
}

sgx_status run_dev(sgx_kaldi *p, const void *x, size_t batch, size_t n_samples, size_t stride, void *out, hipStream_t s) {
    const size_t m = frames_of(p, n_samples);
    sgx_status st = reserve_dev(p, batch, m);
    if (st != SGX_OK) return st;
    const bool f64 = p->dtype == SGX_F64;
    const sgx_kaldi_params &kp = p->p;
    KaldiArgs a{};
    a.x = x; a.out = out; a.win = p->d_win; a.tw = p->d_tw;
    a.band = p->d_band.as<unsigned>(); a.bval = p->d_bval; a.dct = p->d_dct; a.lifter = p->d_lifter;
    a.sample_stride = stride; a.n_samples = n_samples; a.m = m;
    a.batch = unsigned(batch); a.N = unsigned(p->N); a.shift = unsigned(p->shift);
    a.bins = unsigned(p->bins); a.num_ceps = unsigned(p->num_ceps); a.n_out = unsigned(p->n_out); a.nval = unsigned(p->nval);
    a.snip_edges = kp.snip_edges != 0; a.remove_dc = kp.remove_dc_offset != 0; a.raw_energy = kp.raw_energy != 0;
    a.use_energy = kp.use_energy != 0; a.htk_compat = kp.htk_compat != 0;
    a.use_power = p->num_ceps ? 1 : kp.use_power != 0;
    a.use_log = p->num_ceps ? 1 : kp.use_log_fbank != 0;
    a.has_floor = kp.energy_floor > 0.0;
    a.log_floor = a.has_floor ? std::log(kp.energy_floor) : 0.0;
    a.preemph = kp.preemphasis_coefficient != 0.0;
    a.alpha = kp.preemphasis_coefficient;
    a.eps = f64 ? 2.220446049250313e-16 : 1.1920928955078125e-07;
    if (p->fused) {
        a.tile = p->tile; a.sub = p->sub; a.tiles = unsigned((m + p->tile - 1) / p->tile);
        SGX_TRY_HIP(p, launch_fused(p, a, s));
    } else {
        const size_t total = batch * m, gc = gen_chunk(p, total);
        sgx_plan *fft = p->fft.get();
        for (size_t q0 = 0; q0 < total; q0 += gc) {
            const size_t rows = std::min(gc, total - q0);
            SGX_TRY_HIP(p, f64 ? run_generic_chunk<double>(p, a, q0, rows, 0, s) : run_generic_chunk<float>(p, a, q0, rows, 0, s));
            if (sgx_execute(fft, p->d_seg, rows, p->P, p->P, p->d_spec, rows * p->nb * 2, SGX_MEM_DEVICE, s) != SGX_OK)
                return fail(p, SGX_BACKEND, sgx_last_error(fft));
            SGX_TRY_HIP(p, f64 ? run_generic_chunk<double>(p, a, q0, rows, 1, s) : run_generic_chunk<float>(p, a, q0, rows, 1, s));
        }
    }
    if (kp.subtract_mean) {
        const unsigned long long total = (unsigned long long)batch * p->n_out;
        if (f64) hipLaunchKernelGGL(k_kaldi_cmn<double>, dim3(grid_for_items(total)), dim3(256), 0, s, (double *)out, (unsigned long long)m, unsigned(p->n_out), total);
        else hipLaunchKernelGGL(k_kaldi_cmn<float>, dim3(grid_for_items(total)), dim3(256), 0, s, (float *)out, (unsigned long long)m, unsigned(p->n_out), total);
        SGX_TRY_HIP(p, hipGetLastError());
    }
    return SGX_OK;
}

const long double kPiL = 3.141592653589793238462643383279502884L;

long double mel_of(long double f) { return 1127.0L * std::log(1.0L + f / 700.0L); }

}  // namespace

extern "C" {

sgx_status sgx_kaldi_create(const sgx_kaldi_params *params, int32_t route, size_t max_scratch_bytes, sgx_kaldi **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_kaldi>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out || !params) return bad("null argument");
    const sgx_kaldi_params &k = *params;
    if (route != SGX_KALDI_ROUTE_AUTO && route != SGX_KALDI_ROUTE_GENERIC) return bad("unknown route");
    if (k.dtype != SGX_F32 && k.dtype != SGX_F64) return bad("dtype must be f32 or f64");
    // what is not offered
    if (k.dither != 0.0) return bad("dither must be 0 (random dither is not offered)");
    if (k.vtln_warp != 1.0) return bad("vtln_warp must be 1 (VTLN is not offered)");
    if (k.spectrogram) return bad("spectrogram must be 0 (kaldi.spectrogram is not offered: a plan has a filterbank)");
    if (k.min_duration != 0.0) return bad("min_duration must be 0 (short rows are a dimension mismatch, not an empty result)");
    if (k.streaming) return bad("streaming must be 0 (push / flush streaming is not offered)");
    // torchaudio's asserts
    if (!(k.sample_frequency > 0.0) || !std::isfinite(k.sample_frequency)) return bad("sample_frequency must be finite and > 0");
    if (!(k.frame_length_ms > 0.0) || !std::isfinite(k.frame_length_ms) || k.sample_frequency * k.frame_length_ms * 0.001 >= 4294967296.0)
        return bad("frame_length must be finite and > 0");
    if (!(k.frame_shift_ms > 0.0) || !std::isfinite(k.frame_shift_ms) || k.sample_frequency * k.frame_shift_ms * 0.001 >= 4294967296.0)
        return bad("frame_shift must be finite and > 0");
    const size_t N = size_t(k.sample_frequency * k.frame_length_ms * 0.001), shift = size_t(k.sample_frequency * k.frame_shift_ms * 0.001);
    if (N < 2) return bad("frame_length: the window size must be at least 2 samples, got " + std::to_string(N));
    if (shift < 1) return bad("frame_shift: the window shift must be at least 1 sample");
    size_t P = N;
    if (k.round_to_power_of_two) {
        P = 1;
        while (P < N) P <<= 1;
    }
    if (P > (size_t(1) << 20)) return bad("frame_length: the padded window size " + std::to_string(P) + " is above 2^20");
    if (k.window_type < SGX_KALDI_WIN_HANNING || k.window_type > SGX_KALDI_WIN_BLACKMAN)
        return bad("window_type must be hanning, hamming, povey, rectangular or blackman");
    if (!std::isfinite(k.blackman_coeff)) return bad("blackman_coeff must be finite");
    if (!(k.preemphasis_coefficient >= 0.0 && k.preemphasis_coefficient <= 1.0)) return bad("preemphasis_coefficient must be in 0 .. 1");
    if (!(k.energy_floor >= 0.0) || !std::isfinite(k.energy_floor)) return bad("energy_floor must be finite and >= 0");
    if (k.num_mel_bins <= 3) return bad("num_mel_bins must be > 3");
    if (k.num_mel_bins > kKaldiMaxBins) return bad("num_mel_bins is unreasonably large (at most " + std::to_string(kKaldiMaxBins) + ")");
    if (k.num_ceps > k.num_mel_bins) return bad("num_ceps must be <= num_mel_bins");
    if (!std::isfinite(k.cepstral_lifter)) return bad("cepstral_lifter must be finite");
    const double nyquist = 0.5 * k.sample_frequency;
    double high = k.high_freq;
    if (!std::isfinite(k.low_freq) || !std::isfinite(high)) return bad("low_freq and high_freq must be finite");
    if (high <= 0.0) high += nyquist;
    if (!(k.low_freq >= 0.0 && k.low_freq < nyquist)) return bad("low_freq must be in 0 .. Nyquist (exclusive)");
    if (!(high > 0.0 && high <= nyquist)) return bad("high_freq must be in (0, Nyquist] (after adding Nyquist to a value <= 0)");
    if (!(k.low_freq < high)) return bad("low_freq must be below high_freq");

    sgx_kaldi *p = new (std::nothrow) sgx_kaldi();
    if (!p) return fail<sgx_kaldi>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->p = k;
    p->N = N; p->shift = shift; p->P = P; p->nb = P / 2 + 1;
    p->bins = k.num_mel_bins; p->num_ceps = k.num_ceps;
    p->n_out = p->num_ceps ? p->num_ceps : p->bins + (k.use_energy ? 1 : 0);
    p->dtype = k.dtype; p->elem = elem_size(k.dtype); p->device = k.device;
    p->max_scratch = max_scratch_bytes ? max_scratch_bytes : kDefaultScratch;

    // tables: extended precision, rounded once to f64
    p->window.resize(N);
    {
        const long double a = 2.0L * kPiL / (long double)(N - 1);
        for (size_t j = 0; j < N; ++j) {
            const long double aj = a * (long double)j;
            long double w = 1.0L;
            switch (k.window_type) {
            case SGX_KALDI_WIN_HANNING: w = 0.5L - 0.5L * std::cos(aj); break;
            case SGX_KALDI_WIN_HAMMING: w = 0.54L - 0.46L * std::cos(aj); break;
            case SGX_KALDI_WIN_POVEY: w = std::pow(0.5L - 0.5L * std::cos(aj), 0.85L); break;
            case SGX_KALDI_WIN_BLACKMAN: {
                const long double c = (long double)k.blackman_coeff;
                w = c - 0.5L * std::cos(aj) + (0.5L - c) * std::cos(2.0L * aj);
                break;
            }
            default: break;
            }
            p->window[j] = double(w);
        }
    }
    p->bank.assign(p->bins * p->nb, 0.0);
    std::vector<unsigned> band(3 * p->bins, 0u);
    std::vector<double> bval;
    {
        const long double mlo = mel_of((long double)k.low_freq), mhi = mel_of((long double)high);
        const long double delta = (mhi - mlo) / (long double)(p->bins + 1);
        const long double bin_hz = (long double)k.sample_frequency / (long double)P;
        std::vector<long double> melk(P / 2);
        for (size_t q = 0; q < P / 2; ++q) melk[q] = mel_of(bin_hz * (long double)q);
        for (size_t b = 0; b < p->bins; ++b) {
            const long double l = mlo + (long double)b * delta, c = mlo + (long double)(b + 1) * delta, r = mlo + (long double)(b + 2) * delta;
            size_t first = 0, last = 0;  // the positive weights [first, last)
            bool any = false;
            for (size_t q = 0; q < P / 2; ++q) {
                const long double up = (melk[q] - l) / (c - l), down = (r - melk[q]) / (r - c);
                const double w = double(std::max(0.0L, std::min(up, down)));
                p->bank[b * p->nb + q] = w;
                if (w > 0.0) {
                    if (!any) first = q;
                    any = true;
                    last = q + 1;
                }
            }
            band[3 * b] = unsigned(first);
            band[3 * b + 1] = unsigned(last - first);
            band[3 * b + 2] = unsigned(bval.size());
            for (size_t q = first; q < last; ++q) bval.push_back(p->bank[b * p->nb + q]);  // (a triangle: no zero inside)
        }
    }
    p->nval = bval.size();
    p->dct.resize(p->num_ceps * p->bins);
    p->lifter.resize(p->num_ceps);
    {
        const long double B = (long double)p->bins, Q = (long double)k.cepstral_lifter;
        for (size_t i = 0; i < p->num_ceps; ++i) {
            const long double si = i == 0 ? std::sqrt(0.5L) : 1.0L;
            for (size_t b = 0; b < p->bins; ++b)
                p->dct[i * p->bins + b] = double(si * std::sqrt(2.0L / B) * std::cos(kPiL / B * ((long double)b + 0.5L) * (long double)i));
            p->lifter[i] = k.cepstral_lifter != 0.0 ? double(1.0L + 0.5L * Q * std::sin(kPiL * (long double)i / Q)) : 1.0;
        }
    }

    p->fused = route == SGX_KALDI_ROUTE_AUTO && P >= 256 && P <= 2048 && (P & (P - 1)) == 0 && p->bins <= kKaldiMaxFusedBins &&
               reg_split_len(unsigned(P), p->dtype, &p->fa, &p->fb, &p->fc) && fused_split_known(p->dtype, p->fa, p->fb, p->fc) &&
               fused_frame_bytes(p) + fused_bank_bytes(p) <= kKaldiLdsMax;
    if (p->fused) {
        const size_t per = fused_frame_bytes(p);
        unsigned sub = 16;
        while (sub > 1 && (sub * per > kKaldiLdsRound || sub * per + fused_bank_bytes(p) > kKaldiLdsMax)) sub >>= 1;
        p->sub = sub;
        p->tile = kKaldiTile;
    }
    auto tables = [&]() -> sgx_status {
        if (!p->fused) {  // (a host-only plan keeps a host-only transform: its checks of the length are the route's)
            const sgx_status st = create_row_fft(p->P, p->dtype, p->device, p->fft);
            if (st != SGX_OK) return fail(p, st, sgx_last_create_error());
            if (p->device != -2) p->device = sgx_plan_device(p->fft.get());
        }
        if (p->device == -2) return SGX_OK;
        if (p->device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        sgx_status st;
        if ((st = upload(p, p->d_win, p->window, p->dtype)) != SGX_OK) return st;
        if ((st = upload(p, p->d_bval, bval, p->dtype)) != SGX_OK) return st;
        if ((st = upload(p, p->d_dct, p->dct, p->dtype)) != SGX_OK) return st;
        if ((st = upload(p, p->d_lifter, p->lifter, p->dtype)) != SGX_OK) return st;
        SGX_TRY_HIP(p, hipMalloc(&p->d_band.ptr, band.size() * sizeof(unsigned)));
        p->d_band.bytes = band.size() * sizeof(unsigned);
        SGX_TRY_HIP(p, hipMemcpy(p->d_band, band.data(), p->d_band.bytes, hipMemcpyHostToDevice));
        if (p->fused) {  // W_P^k rounded once from extended precision, as k_welch's
            std::vector<double> tw(2 * p->P);
            for (size_t q = 0; q < p->P; ++q) {
                const long double a = -2.0L * kPiL * (long double)q / (long double)p->P;
                tw[2 * q] = double(std::cos(a));
                tw[2 * q + 1] = double(std::sin(a));
            }
            if ((st = upload(p, p->d_tw, tw, p->dtype)) != SGX_OK) return st;
        }
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_kaldi_destroy);
}

void sgx_kaldi_destroy(sgx_kaldi *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device >= 0) (void)dg.enter(p->device);
    delete p;
}

size_t sgx_kaldi_window_size(const sgx_kaldi *p) { return p ? p->N : 0; }
size_t sgx_kaldi_window_shift(const sgx_kaldi *p) { return p ? p->shift : 0; }
size_t sgx_kaldi_padded_window_size(const sgx_kaldi *p) { return p ? p->P : 0; }
size_t sgx_kaldi_n_out(const sgx_kaldi *p) { return p ? p->n_out : 0; }
size_t sgx_kaldi_n_frames(const sgx_kaldi *p, size_t n_samples) { return p ? frames_of(p, n_samples) : 0; }

sgx_status sgx_kaldi_window(const sgx_kaldi *p, double *window) {
    if (!p || !window) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->window.begin(), p->window.end(), window);
    return SGX_OK;
}

sgx_status sgx_kaldi_mel_banks(const sgx_kaldi *p, double *banks) {
    if (!p || !banks) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->bank.begin(), p->bank.end(), banks);
    return SGX_OK;
}

sgx_status sgx_kaldi_dct(const sgx_kaldi *p, double *dct) {
    if (!p || !dct) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->dct.begin(), p->dct.end(), dct);
    return SGX_OK;
}

sgx_status sgx_kaldi_lifter(const sgx_kaldi *p, double *lifter) {
    if (!p || !lifter) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::copy(p->lifter.begin(), p->lifter.end(), lifter);
    return SGX_OK;
}

sgx_status sgx_kaldi_reserve(sgx_kaldi *p, size_t batch, size_t n_samples, int32_t host_staging) {
    if (!p || batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (n_samples < p->N) return dim_mismatch(p, p->N, n_samples, " (n_samples must be at least the window size)");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    const size_t m = frames_of(p, n_samples);
    if ((st = reserve_dev(p, batch, m)) != SGX_OK) return st;
    if (host_staging) {
        if ((st = kgrow(p, p->d_in, batch * n_samples * p->elem)) != SGX_OK) return st;
        if ((st = kgrow(p, p->d_out, batch * m * p->n_out * p->elem)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_kaldi_execute(sgx_kaldi *p, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out, size_t out_elems,
                             int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!x || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (n_samples < p->N) return dim_mismatch(p, p->N, n_samples, " (n_samples must be at least the window size)");
    if (sample_stride < n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    const size_t m = frames_of(p, n_samples);
    if (batch > 0xffffffffull || n_samples > (size_t(1) << 40) || m >= 0x7fffffffull || ((m + kKaldiTile - 1) / kKaldiTile) * batch >= 0x7fffffffull)
        return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
    if (out_elems != batch * m * p->n_out) return dim_mismatch(p, batch * m * p->n_out, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return run_dev(p, x, batch, n_samples, sample_stride, out, s);
    const size_t in_bytes = ((batch - 1) * sample_stride + n_samples) * p->elem, out_bytes = out_elems * p->elem;
    sgx_status st;
    if ((st = kgrow(p, p->d_in, in_bytes)) != SGX_OK) return st;
    if ((st = kgrow(p, p->d_out, out_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
    if ((st = run_dev(p, p->d_in, batch, n_samples, sample_stride, p->d_out, s)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

size_t sgx_kaldi_allocations(const sgx_kaldi *p) { return p ? p->allocations : 0; }
size_t sgx_kaldi_tile(const sgx_kaldi *p) { return p && p->fused ? p->tile : 0; }
const char *sgx_kaldi_kernel_name(const sgx_kaldi *p) { return !p ? "" : p->fused ? "k_kaldi" : "kaldi_generic"; }
int32_t sgx_kaldi_device(const sgx_kaldi *p) { return p ? p->device : -2; }
const char *sgx_kaldi_last_error(const sgx_kaldi *p) { return p ? p->err.c_str() : create_err<sgx_kaldi>().c_str(); }

}  // extern "C"

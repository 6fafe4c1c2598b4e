// mdct.hip — batched MDCT / IMDCT plans of libspectro_hip.so (C ABI: sgx_mdct_* in include/spectro_hip.h), kernels and host side.
//
// Reference: src/mdct.rs (MdctParams :54-140, mdct :387-440, imdct :442-497).  With 2N = window_size, z = x w (one frame):
//   C[k] = sum_{n < 2N} z[n] cos(pi (2n + 1 + N)(2k + 1) / (4N)),  k < N
//   y[m] = (2/N) sum_{k < N} C[k] cos(pi (2m + 1 + N)(2k + 1) / (4N)),  m < 2N, then y w overlap-added at f hop, no normalisation.
//
// N even (M = N / 2, h = N / 2): the MDCT is the DCT-IV of the fold r = (-c_R - d, a - b_R) of the quarters (a, b, c, d) of z,
//   r[m] = (m < h ? -z[3h + m] : z[m - h]) - z[3h - 1 - m],
// and a DCT-IV of length N is one M-point complex transform:
//   c[n] = (r[2n] + i r[N-1-2n]) t1[n],  t1[n] = e^(-i pi (4n + 1) / (4N));   Y = DFT_M(c);   y[k] = Y[k] t2[k],  t2[k] = e^(-i pi k / N)
//   X[2k] = Re y[k],  X[N-1-2k] = -Im y[k].
// The IMDCT runs the same DCT-IV on the coefficients (scale 2/N folded into t2) and unfolds u = DCT-IV(C) into the 2N outputs:
//   y[m] = U[m + h],  U[p] = u[p] (p < N), -u[2N-1-p] (N <= p < 2N), -u[p-2N] (p >= 2N).
// N odd (generic route only): with g[n] = z[n] e^(-i pi n / (2N)), G = DFT_2N(g) splits into two N-point transforms
//   E = DFT_N(g[n] + g[n+N]),  O = DFT_N((g[n] - g[n+N]) e^(-i pi n / N));  C[2q] = Re(phi_2q E[q]),  C[2q+1] = Re(phi_2q+1 O[q]),
//   phi_k = e^(-i pi (1 + N)(2k + 1) / (4N));
// and for the inverse, with m' = m + (N+1)/2 and m'' = m' mod 2N:  E = DFT_N(C),  O = DFT_N(C[k] e^(-i pi k / N)),
//   y[m] = Re(psi_m H[m'']),  H[2q] = E[q], H[2q+1] = O[q],  psi_m = (2/N) e^(-i pi m' / (2N)).
//
// Routes:
//   k_mdct_fwd<T, A, B, C>   fused forward for N even whose M has a reg_split_len split: a workgroup takes a tile of F consecutive
//                            frames of one signal; the fold windows and pre-twiddles the samples into LDS (each sample of a frame
//                            feeds exactly one of its M complex values), the M-point transform runs as the passes of k_c2c_reg,
//                            and the post-twiddle reads the result out of LDS with lanes over frames: every coefficient row gets F
//                            consecutive frames per store ([batch][N][n_frames], frames contiguous).
//   k_imdct_ola<T, A, B, C>  fused inverse for hop == N on the same splits: a tile of F frames (the first a halo, recomputed by the previous
//                            tile) reads the coefficients F frames wide per row, transforms, and writes the F - 1 hop blocks it owns with
//                            contiguous stores; block P / N is frame P / N (first half) plus frame P / N - 1 (second half), added in
//                            ascending frame order as the reference adds them.
//   generic                  every other shape: k_mdct_fold -> the batched complex dispatch (register-tiled, else chirp-z, else the LDS
//                            tile kernel; lengths below 16 are summed directly in the post kernel) -> k_mdct_post -> (inverse) k_mdct_ola,
//                            over chunks of at most kChunkBytes of scratch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "rr_passes.h"
#include "plan_host.h"
#include "xcd_map.h"

using namespace sgx;

namespace {

constexpr double kPiM = 3.14159265358979323846264338327950288;
constexpr size_t kMdctLds = 72 * 1024;           // LDS per workgroup of the fused kernels: two workgroups per CU
constexpr size_t kChunkBytes = size_t(256) << 20;  // generic route: scratch per buffer; a call is cut into chunks of frames
constexpr size_t kMaxWindow = 8192, kMaxWindowPow2 = 16384;

struct MdctArgs {
    const void *in;   // forward: samples [batch][n_samples]; inverse: coefficients [batch][N][n_frames]
    void *out;        // forward: coefficients [batch][N][n_frames]; inverse: signal [batch][out_len]
    const void *win;  // [2N] T
    const void *t1;   // [M] complex T: pre-twiddle
    const void *t2;   // [M] complex T: post-twiddle (inverse: times 2/N)
    const void *tw;   // [M] complex T: W_M^k
    unsigned long long n_samples, out_len;
    unsigned batch, hop, n_frames, tiles, nbk;
};

// waves per SIMD the register allocation aims at: a 72 KB tile leaves room for two workgroups per CU, i.e. two waves per SIMD, so the
// f32 instances take the 256 registers of that occupancy (the fold of pass 1 holds four samples and four window values per point)
template <typename T, int A_, int B_, int C_>
constexpr unsigned mdct_waves() { return rr_waves<T, A_, B_, C_>() < 2 ? rr_waves<T, A_, B_, C_>() : 2; }

template <typename T, int A_, int B_, int C_>
__global__ __launch_bounds__(256, (mdct_waves<T, A_, B_, C_>())) void k_mdct_fwd(MdctArgs a, unsigned ltile) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, BC = B_ * C_, M = A * BC, N = 2 * M, h = M;
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned FS = L::FS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    V *buf = (V *)smem;  // [tile][FS]
    const unsigned tid = threadIdx.x, tile = 1u << ltile;
    const unsigned lb = xcd_logical_block(a.tiles * a.batch);  // neighbouring tiles share sample lines: keep them in one XCD
    if (lb >= a.tiles * a.batch) return;
    const unsigned t = lb % a.tiles, b = lb / a.tiles;
    const unsigned f0 = t * tile, nf = min(tile, a.n_frames - f0);
    const T *xt = (const T *)a.in + (size_t)b * a.n_samples + (size_t)f0 * a.hop;
    const T *w = (const T *)a.win;
    const V *t1 = (const V *)a.t1, *t2 = (const V *)a.t2, *tw = (const V *)a.tw;

    // fold: lanes along the frame, c[n] = (r[2n] + i r[N-1-2n]) t1[n] from the 4 samples that feed it, into the row in natural order
    // (held in LDS rather than in the registers of pass 1: with all A points' samples and window values in flight the long-pass
    // instances spill)
#pragma unroll 1
    for (unsigned idx = tid; idx < nf * M; idx += 256) {
        const unsigned n = idx % M, s = idx / M;
        const unsigned so = s * a.hop;  // 32-bit offsets from the tile's (uniform) first sample
        auto z = [&](unsigned i) { return xt[so + i] * w[i]; };
        // r[m]: one sample picked by the branch (a select of the index, not of two loads), one subtracted
        auto rf = [&](unsigned m) { const bool lo = m < h; return (lo ? T(-1) : T(1)) * z(lo ? 3u * h + m : m - h) - z(3u * h - 1u - m); };
        buf[(size_t)s * FS + n] = inreg::cmulv((V){rf(2u * n), rf(N - 1u - 2u * n)}, t1[n]);
    }
    // pass 1 from LDS in rounds of whole rows: a round reads its rows completely before it overwrites them in the pass's layout
    constexpr unsigned RPR = 256u / BC;  // rows per round
    for (unsigned row0 = 0; row0 < nf; row0 += RPR) {
        const unsigned s = row0 + tid / BC, r = tid % BC;
        const bool act = tid < RPR * BC && s < nf;
        V v[A];
        __syncthreads();
        if (act) {
#pragma unroll
            for (unsigned n1 = 0; n1 < A; ++n1) v[n1] = buf[(size_t)s * FS + BC * n1 + r];
        }
        __syncthreads();
        if (act) rr_pass1_store<T, A_, B_, C_>(v, buf + (size_t)s * FS, r, tw);
    }
    rr_passes23<T, A_, B_, C_>(buf, nf, tid, tw);
    // post-twiddle; lanes over frames: coefficient row j takes the tile's nf frames in one run of stores
    T *out = (T *)a.out + (size_t)b * N * a.n_frames + f0;
#pragma unroll 1
    for (unsigned idx = tid; idx < tile * N; idx += 256) {
        const unsigned s = idx & (tile - 1u), j = idx >> ltile;
        if (s >= nf) continue;
        const unsigned k = (j & 1u) ? (N - 1u - j) >> 1 : j >> 1;
        const V y = inreg::cmulv(buf[(size_t)s * FS + L::of_output(k)], t2[k]);
        out[(size_t)j * a.n_frames + s] = (j & 1u) ? -y.y : y.x;
    }
}

template <typename T, int A_, int B_, int C_>
__global__ __launch_bounds__(256, (mdct_waves<T, A_, B_, C_>())) void k_imdct_ola(MdctArgs a, unsigned ltile) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, BC = B_ * C_, M = A * BC, N = 2 * M, h = M;
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned FS = L::FS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    V *buf = (V *)smem;  // [tile][FS]
    const unsigned tid = threadIdx.x, tile = 1u << ltile;
    const unsigned lb = xcd_logical_block(a.tiles * a.batch);
    if (lb >= a.tiles * a.batch) return;
    const unsigned t = lb % a.tiles, b = lb / a.tiles;
    // row rr of the tile is frame fbase + rr; the tile owns hop blocks [t nbk, (t + 1) nbk), which need frames t nbk - 1 .. (t + 1) nbk - 1
    const long long blk0 = (long long)t * a.nbk, fbase = blk0 - 1;
    const T *cin = (const T *)a.in + (size_t)b * N * a.n_frames;
    const T *w = (const T *)a.win;
    const V *t1 = (const V *)a.t1, *t2 = (const V *)a.t2, *tw = (const V *)a.tw;

    // pass 1: lanes over frames (the [bin][frame] rows are read tile frames wide); frames outside the signal transform zeros
#pragma unroll 1
    for (unsigned idx = tid; idx < tile * BC; idx += 256) {
        const unsigned rr = idx & (tile - 1u), r = idx >> ltile;
        const long long f = fbase + rr;
        const bool ok = f >= 0 && f < (long long)a.n_frames;
        const T *cf = cin + (ok ? (size_t)f : 0);
        V v[A];
#pragma unroll
        for (unsigned n1 = 0; n1 < A; ++n1) {
            const unsigned n = BC * n1 + r;
            const V c = ok ? (V){cf[(size_t)(2u * n) * a.n_frames], cf[(size_t)(N - 1u - 2u * n) * a.n_frames]} : (V){T(0), T(0)};
            v[n1] = inreg::cmulv(c, t1[n]);
        }
        rr_pass1_store<T, A_, B_, C_>(v, buf + (size_t)rr * FS, r, tw);
    }
    rr_passes23<T, A_, B_, C_>(buf, tile, tid, tw);
    // frame sample m of row rr: y[m] = U[m + h] (unfolded DCT-IV, 2/N in t2)
    auto y = [&](unsigned rr, unsigned m) {
        const unsigned p = m + h;
        const unsigned up = p < N ? p : (p < 2u * N ? 2u * N - 1u - p : p - 2u * N);
        const unsigned k = (up & 1u) ? (N - 1u - up) >> 1 : up >> 1;
        const V yv = inreg::cmulv(buf[(size_t)rr * FS + L::of_output(k)], t2[k]);
        const T u = (up & 1u) ? -yv.y : yv.x;
        return p < N ? u : -u;
    };
    T *out = (T *)a.out + (size_t)b * a.out_len;
    const unsigned long long p0 = (unsigned long long)blk0 * N;
#pragma unroll 1
    for (unsigned i = tid; i < a.nbk * N; i += 256) {
        const unsigned long long pos = p0 + i;
        if (pos >= a.out_len) break;
        const unsigned rr = i / N + 1u, j = i % N;
        const long long blk = blk0 + (long long)(rr - 1u);
        T acc = T(0);
        if (blk >= 1) acc += y(rr - 1u, j + N) * w[j + N];
        if (blk < (long long)a.n_frames) acc += y(rr, j) * w[j];
        out[pos] = acc;
    }
}

template <typename T, int A, int B, int C>
hipError_t launch_fused_t(const MdctArgs &a, bool inverse, unsigned ltile, size_t lds, hipStream_t s) {
    const void *fn = inverse ? (const void *)k_imdct_ola<T, A, B, C> : (const void *)k_mdct_fwd<T, A, B, C>;
    if (lds > 64 * 1024) {
        const hipError_t e = set_max_dynamic_lds(fn, (int)kMdctLds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid(xcd_grid((unsigned long long)a.tiles * a.batch));
    if (inverse) hipLaunchKernelGGL((k_imdct_ola<T, A, B, C>), grid, dim3(256), lds, s, a, ltile);
    else hipLaunchKernelGGL((k_mdct_fwd<T, A, B, C>), grid, dim3(256), lds, s, a, ltile);
    return hipGetLastError();
}

// LDS bytes of one frame of the fused kernels' tile, 0 if M has no pass split
size_t fused_frame_bytes(unsigned M, int dtype, unsigned *fa, unsigned *fb, unsigned *fc) {
    if (!reg_split_len(M, dtype, fa, fb, fc)) return 0;
    const size_t es = elem_size(dtype);
    return rr_seq_bytes(2 * (unsigned)es, *fa, *fb, *fc);
}

// log2 of the fused kernels' frames per tile: the largest power of two up to 32 within kMdctLds; -1: not fused.  The forward tile
// shrinks to the signal's frame count (the result does not depend on the tile).
int fused_ltile(unsigned M, int dtype, unsigned n_frames, bool inverse) {
    unsigned fa, fb, fc;
    const size_t per = fused_frame_bytes(M, dtype, &fa, &fb, &fc);
    if (per == 0 || per > kMdctLds) return -1;
    int lt = 5;
    while (lt > 0 && ((size_t(1) << lt) * per > kMdctLds || (!inverse && n_frames && (1u << (lt - 1)) >= n_frames))) --lt;
    return lt;
}

hipError_t launch_fused(const MdctArgs &a0, unsigned M, int dtype, bool inverse, hipStream_t s) {
    unsigned fa, fb, fc;
    const size_t per = fused_frame_bytes(M, dtype, &fa, &fb, &fc);
    const int lt = fused_ltile(M, dtype, a0.n_frames, inverse);
    if (lt < 0 || (inverse && lt < 2)) return hipErrorNotSupported;
    MdctArgs a = a0;
    const unsigned tile = 1u << lt;
    if (inverse) {
        a.nbk = tile - 1u;
        const unsigned long long blocks = (unsigned long long)a.n_frames + 1u;  // out_len = (n_frames + 1) N
        a.tiles = (unsigned)((blocks + a.nbk - 1u) / a.nbk);
    } else {
        a.tiles = (a.n_frames + tile - 1u) / tile;
    }
    const unsigned long long g = (unsigned long long)a.tiles * a.batch;
    if (g == 0 || g >= 0x7fffffffull) return hipErrorInvalidConfiguration;
    const size_t lds = (size_t)tile * per;
#define SGX_MDCT_F32(A, B, C) if (fa == A && fb == B && fc == C) return launch_fused_t<float, A, B, C>(a, inverse, (unsigned)lt, lds, s);
#define SGX_MDCT_F64(A, B, C) if (fa == A && fb == B && fc == C) return launch_fused_t<double, A, B, C>(a, inverse, (unsigned)lt, lds, s);
    if (dtype == SGX_F64) {
        SGX_RR_SPLITS_F64(SGX_MDCT_F64)
        SGX_RR_SPLITS_MIXED(SGX_MDCT_F64)
    } else {
        SGX_RR_SPLITS_F32(SGX_MDCT_F32)
        SGX_RR_SPLITS_MIXED(SGX_MDCT_F32)
    }
#undef SGX_MDCT_F32
#undef SGX_MDCT_F64
    return hipErrorNotSupported;
}

// ---- generic route -------------------------------------------------------------------------------------------------------------
// A chunk is `gc` consecutive frames of the flattened (signal, frame) index g = b n_frames + f, starting at g0.  Sequences of length
// L in the complex scratch: N even one per frame (L = M), N odd two per frame (E then O, L = N).
struct GenArgs {
    const void *in;
    void *out;
    const void *win;                  // [2N] T
    const void *pa, *pb;              // fold tables: N even t1 [M] (pb unused); N odd e^(-i pi n / 2N) [2N] and e^(-i pi n / N) [N]
    const void *post;                 // N even t2 [M] (inverse: 2/N t2); N odd phi [N] (forward) / psi [2N] (inverse)
    void *seq;                        // fold output / transform input [gc][spf][L]
    const void *spec;                 // transform output (seq itself when the lengths are summed directly)
    void *frames;                     // inverse: windowed frames [gc][2N]
    unsigned long long n_samples, out_len, g0, gc;
    unsigned N, hop, n_frames, L, direct;
};

template <typename T>
__global__ __launch_bounds__(256) void k_mdct_fold(GenArgs a, int inverse) {
    typedef typename PairOf<T>::type V;
    const unsigned N = a.N, L = a.L;
    const bool odd = N & 1u;
    const unsigned long long total = a.gc * (odd ? 2ull : 1ull) * L;
    const T *w = (const T *)a.win;
    const V *pa = (const V *)a.pa, *pb = (const V *)a.pb;
    V *seq = (V *)a.seq;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        // consecutive threads: consecutive frames of the chunk (inverse: contiguous coefficient reads) or points (forward)
        unsigned long long gl;
        unsigned n, part = 0;
        if (inverse) {
            gl = i % a.gc;
            const unsigned long long q = i / a.gc;
            n = (unsigned)(q % L);
            part = (unsigned)(q / L);
        } else {
            n = (unsigned)(i % L);
            const unsigned long long q = i / L;
            part = odd ? (unsigned)(q & 1u) : 0u;
            gl = odd ? q >> 1 : q;
        }
        const unsigned long long g = a.g0 + gl, b = g / a.n_frames, f = g % a.n_frames;
        V v;
        if (!inverse) {
            const T *xf = (const T *)a.in + b * a.n_samples + f * a.hop;
            auto z = [&](unsigned j) { return xf[j] * w[j]; };
            if (!odd) {
                const unsigned h = N / 2;
                auto rf = [&](unsigned m) { return (m < h ? -z(3u * h + m) : z(m - h)) - z(3u * h - 1u - m); };
                v = inreg::cmulv((V){rf(2u * n), rf(N - 1u - 2u * n)}, pa[n]);
            } else {
                const V g1 = pa[n] * z(n), g2 = pa[n + N] * z(n + N);
                v = part ? inreg::cmulv(g1 - g2, pb[n]) : g1 + g2;
            }
        } else {
            const T *cb = (const T *)a.in + b * N * a.n_frames + f;
            if (!odd) {
                v = inreg::cmulv((V){cb[(size_t)(2u * n) * a.n_frames], cb[(size_t)(N - 1u - 2u * n) * a.n_frames]}, pa[n]);
            } else {
                const T c = cb[(size_t)n * a.n_frames];
                v = part ? pb[n] * c : (V){c, T(0)};
            }
        }
        seq[(gl * (odd ? 2u : 1u) + part) * L + n] = v;
    }
}

// transform output element k of sequence sq (a direct sum over the fold output for lengths below 16)
template <typename T>
__device__ __forceinline__ typename PairOf<T>::type gen_spec(const GenArgs &a, unsigned long long sq, unsigned k) {
    typedef typename PairOf<T>::type V;
    if (!a.direct) return ((const V *)a.spec)[sq * a.L + k];
    const V *s = (const V *)a.seq + sq * a.L;
    V acc = (V){T(0), T(0)};
    for (unsigned n = 0; n < a.L; ++n) {
        const double ang = -2.0 * kPiM * double((unsigned long long)n * k % a.L) / double(a.L);
        acc = acc + inreg::cmulv(s[n], (V){T(cos(ang)), T(sin(ang))});
    }
    return acc;
}

template <typename T>
__global__ __launch_bounds__(256) void k_mdct_post(GenArgs a, int inverse) {
    typedef typename PairOf<T>::type V;
    const unsigned N = a.N;
    const bool odd = N & 1u;
    const V *post = (const V *)a.post;
    const T *w = (const T *)a.win;
    const unsigned long long per = inverse ? 2ull * N : N, total = a.gc * per;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        if (!inverse) {
            // lanes over the chunk's frames: row j of the [batch][N][n_frames] output in runs of consecutive frames
            const unsigned long long gl = i % a.gc, g = a.g0 + gl, b = g / a.n_frames, f = g % a.n_frames;
            const unsigned j = (unsigned)(i / a.gc);
            T val;
            if (!odd) {
                const unsigned k = (j & 1u) ? (N - 1u - j) >> 1 : j >> 1;
                const V y = inreg::cmulv(gen_spec<T>(a, gl, k), post[k]);
                val = (j & 1u) ? -y.y : y.x;
            } else {
                const V y = inreg::cmulv(gen_spec<T>(a, gl * 2u + (j & 1u), j >> 1), post[j]);
                val = y.x;
            }
            ((T *)a.out)[(b * N + j) * a.n_frames + f] = val;
        } else {
            const unsigned long long gl = i / per;
            const unsigned m = (unsigned)(i % per);
            T val;
            if (!odd) {
                const unsigned h = N / 2, p = m + h;
                const unsigned up = p < N ? p : (p < 2u * N ? 2u * N - 1u - p : p - 2u * N);
                const unsigned k = (up & 1u) ? (N - 1u - up) >> 1 : up >> 1;
                const V y = inreg::cmulv(gen_spec<T>(a, gl, k), post[k]);
                const T u = (up & 1u) ? -y.y : y.x;
                val = p < N ? u : -u;
            } else {
                const unsigned m2 = (m + (N + 1u) / 2u) % (2u * N);
                val = inreg::cmulv(gen_spec<T>(a, gl * 2u + (m2 & 1u), m2 >> 1), post[m]).x;
            }
            ((T *)a.frames)[gl * per + m] = val * w[m];
        }
    }
}

// overlap-add of the chunk's windowed frames into out[batch][out_len] (zeroed before the first chunk): every position adds the chunk's
// frames that cover it in ascending frame order, on top of what the earlier chunks left there
template <typename T>
__global__ __launch_bounds__(256) void k_mdct_ola(GenArgs a, unsigned long long b0, unsigned long long nsig) {
    const unsigned n2 = 2u * a.N;
    const unsigned long long total = nsig * a.out_len;
    const T *fr = (const T *)a.frames;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long b = b0 + i / a.out_len, pos = i % a.out_len;
        const unsigned long long gb = b * a.n_frames;  // this signal's first global frame
        // frames f with f hop <= pos < f hop + 2N, inside the chunk
        long long f_lo = pos >= n2 ? (long long)((pos - n2) / a.hop + 1) : 0;
        long long f_hi = (long long)(pos / a.hop);
        f_hi = std::min(f_hi, (long long)a.n_frames - 1);
        f_lo = std::max(f_lo, (long long)a.g0 - (long long)gb);
        f_hi = std::min(f_hi, (long long)(a.g0 + a.gc) - 1 - (long long)gb);
        if (f_lo > f_hi) continue;
        T *o = (T *)a.out + b * a.out_len + pos;
        T acc = *o;
        for (long long f = f_lo; f <= f_hi; ++f) acc += fr[(gb + f - a.g0) * n2 + (pos - (unsigned long long)f * a.hop)];
        *o = acc;
    }
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_mdct {
    size_t two_n = 0, n = 0, hop = 0;
    int dtype = SGX_F32, device = -1;
    size_t elem = 4;
    int window_kind = 0;
    double window_param = 0.0;
    std::vector<double> custom, window;
    bool fused_fwd = false, fused_inv = false;
    unsigned L = 0;  // generic route: transform length
    DevBuf d_win, d_t1, d_t2, d_t2i, d_tw;       // fused and generic (N even)
    DevBuf d_pa, d_pb, d_phi, d_psi, d_twL;      // generic, N odd (twL: W_L, L = N)
    BsDevTables bs;
    DevBuf d_seq, d_spec, d_frames, d_in, d_out;
    mutable std::string err;
};

namespace {

// e^(i ang(k)) for k < n, interleaved, times `scale`
template <typename F>
std::vector<double> ctab(size_t n, double scale, F ang) {
    std::vector<double> t(2 * n);
    for (size_t k = 0; k < n; ++k) {
        const double a = ang(double(k));
        t[2 * k] = scale * std::cos(a);
        t[2 * k + 1] = scale * std::sin(a);
    }
    return t;
}

size_t frames_of(const sgx_mdct *p, size_t n_samples) { return n_samples < p->two_n ? 0 : (n_samples - p->two_n) / p->hop + 1; }
size_t inv_len(const sgx_mdct *p, size_t n_frames) { return n_frames ? p->hop * n_frames + p->two_n - p->hop : 0; }

// generic route: frames per chunk and the scratch it needs
struct GenSizes {
    size_t gc, seq, frames;
};
GenSizes gen_sizes(const sgx_mdct *p, size_t total_frames, bool inverse) {
    const size_t spf = (p->n & 1) ? 2 : 1;
    const size_t per_seq = spf * p->L * 2 * p->elem, per_frame = inverse ? p->two_n * p->elem : 0;
    const size_t gc = std::max<size_t>(1, std::min(total_frames, kChunkBytes / std::max(per_seq, per_frame)));
    return {gc, gc * per_seq, gc * per_frame};
}

sgx_status gen_reserve(sgx_mdct *p, size_t total_frames, bool inverse) {
    const GenSizes z = gen_sizes(p, total_frames, inverse);
    sgx_status st;
    if ((st = grow(p, p->d_seq, z.seq)) != SGX_OK) return st;
    if (p->L >= 16 && (st = grow(p, p->d_spec, z.seq)) != SGX_OK) return st;
    if (inverse && (st = grow(p, p->d_frames, z.frames)) != SGX_OK) return st;
    return SGX_OK;
}

sgx_status run_generic(sgx_mdct *p, const void *in, size_t batch, size_t n_samples, size_t n_frames, void *out, bool inverse, hipStream_t s) {
    const size_t total = batch * n_frames;
    sgx_status st = gen_reserve(p, total, inverse);
    if (st != SGX_OK) return st;
    const GenSizes z = gen_sizes(p, total, inverse);
    const bool odd = p->n & 1;
    GenArgs a{};
    a.in = in; a.out = out; a.win = p->d_win;
    a.pa = odd ? p->d_pa : p->d_t1; a.pb = p->d_pb;
    a.post = odd ? (inverse ? p->d_psi : p->d_phi) : (inverse ? p->d_t2i : p->d_t2);
    a.seq = p->d_seq; a.frames = p->d_frames;
    a.direct = p->L < 16;
    a.spec = a.direct ? p->d_seq : p->d_spec;
    a.n_samples = n_samples; a.out_len = inv_len(p, n_frames);
    a.N = unsigned(p->n); a.hop = unsigned(p->hop); a.n_frames = unsigned(n_frames); a.L = p->L;
    if (inverse) SGX_TRY_HIP(p, hipMemsetAsync(out, 0, batch * a.out_len * p->elem, s));
    const bool f64 = p->dtype == SGX_F64;
    for (size_t g0 = 0; g0 < total; g0 += z.gc) {
        a.g0 = g0;
        a.gc = std::min(z.gc, total - g0);
        const unsigned long long nseq = a.gc * (odd ? 2u : 1u);
        const unsigned long long fold_total = nseq * p->L;
        if (f64) hipLaunchKernelGGL(k_mdct_fold<double>, dim3(grid_for_items(fold_total)), dim3(256), 0, s, a, int(inverse));
        else hipLaunchKernelGGL(k_mdct_fold<float>, dim3(grid_for_items(fold_total)), dim3(256), 0, s, a, int(inverse));
        SGX_TRY_HIP(p, hipGetLastError());
        if (!a.direct) {
            C2cArgs c{};
            c.in = p->d_seq; c.out = p->d_spec;
            c.n = p->L;
            c.log2n = 0;
            if ((p->L & (p->L - 1)) == 0) while ((1u << c.log2n) < p->L) ++c.log2n;
            c.nseq = unsigned(nseq); c.batch = 1;
            c.in_img = c.out_img = 0;
            c.in_ss = c.out_ss = p->L; c.in_is = c.out_is = 1;
            c.tw = odd ? p->d_twL : p->d_tw; c.inverse = 0; c.in_seq_fast = 0; c.out_seq_fast = 0; c.scale = 1.0;
            c.tile = fft2d_tile_for(p->L, p->dtype);
            c.tiles = c.tile ? unsigned((nseq + c.tile - 1) / c.tile) : 0;
            hipError_t e = launch_c2c_reg(c, p->dtype, s);
            if (e == hipErrorNotSupported && p->bs.M) e = launch_c2c_bluestein(c, p->bs, p->dtype, s);
            if (e == hipErrorNotSupported) e = launch_c2c_tile(c, p->dtype, s);
            SGX_TRY_HIP(p, e);
        }
        const unsigned long long post_total = a.gc * (inverse ? 2ull * p->n : p->n);
        if (f64) hipLaunchKernelGGL(k_mdct_post<double>, dim3(grid_for_items(post_total)), dim3(256), 0, s, a, int(inverse));
        else hipLaunchKernelGGL(k_mdct_post<float>, dim3(grid_for_items(post_total)), dim3(256), 0, s, a, int(inverse));
        SGX_TRY_HIP(p, hipGetLastError());
        if (inverse) {
            const unsigned long long b0 = g0 / n_frames, b1 = (g0 + a.gc - 1) / n_frames, nsig = b1 - b0 + 1;
            if (f64) hipLaunchKernelGGL(k_mdct_ola<double>, dim3(grid_for_items(nsig * a.out_len)), dim3(256), 0, s, a, b0, nsig);
            else hipLaunchKernelGGL(k_mdct_ola<float>, dim3(grid_for_items(nsig * a.out_len)), dim3(256), 0, s, a, b0, nsig);
            SGX_TRY_HIP(p, hipGetLastError());
        }
    }
    return SGX_OK;
}

sgx_status run_dev(sgx_mdct *p, const void *in, size_t batch, size_t n_samples, size_t n_frames, void *out, bool inverse, hipStream_t s) {
    if ((inverse ? p->fused_inv : p->fused_fwd)) {
        MdctArgs a{};
        a.in = in; a.out = out; a.win = p->d_win; a.t1 = p->d_t1; a.t2 = inverse ? p->d_t2i : p->d_t2; a.tw = p->d_tw;
        a.n_samples = n_samples; a.out_len = inv_len(p, n_frames);
        a.batch = unsigned(batch); a.hop = unsigned(p->hop); a.n_frames = unsigned(n_frames);
        const hipError_t e = launch_fused(a, unsigned(p->n / 2), p->dtype, inverse, s);
        if (e != hipErrorNotSupported) {
            SGX_TRY_HIP(p, e);
            return SGX_OK;
        }
    }
    return run_generic(p, in, batch, n_samples, n_frames, out, inverse, s);
}

}  // namespace

namespace {

sgx_status validate(size_t w, size_t hop, int32_t kind, const double *custom, uint32_t custom_len, int32_t dtype, std::string &msg) {
    auto bad = [&](const std::string &m) { msg = "Invalid input: " + m; return SGX_INVALID_INPUT; };
    if (w % 2 != 0) return bad("window_size must be even, got " + std::to_string(w));  // src/mdct.rs:75-86
    if (w < 4) return bad("window_size must be >= 4, got " + std::to_string(w));
    if (hop == 0) return bad("hop_size must be > 0");
    if (kind < SGX_WIN_RECTANGULAR || kind > SGX_WIN_CUSTOM) return bad("unknown window type");
    // (the reference panics in make_window on a custom window of another length; here it is an error)
    if (kind == SGX_WIN_CUSTOM && (!custom || custom_len != w))
        return bad("Custom window size (" + std::to_string(custom ? custom_len : 0) + ") must match window_size (" + std::to_string(w) + ")");
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    if (w > kMaxWindowPow2 || (w > kMaxWindow && (w & (w - 1)) != 0)) {
        msg = "hip -- FFT backend error: window_size " + std::to_string(w) +
              " is not supported (every even size up to 8192 and the powers of two up to 16384)";
        return SGX_BACKEND;
    }
    if (hop > 0x7fffffffull) return bad("hop_size too large");
    return SGX_OK;
}

sgx_status with_staging(sgx_mdct *p, const void *in, size_t in_bytes, void *out, size_t out_bytes, int mem_kind, hipStream_t s,
                        const std::function<sgx_status(const void *, void *)> &body);

}  // namespace

extern "C" {

sgx_status sgx_mdct_create(size_t window_size, size_t hop_size, int32_t window_kind, double window_param, const double *custom_window,
                           uint32_t custom_window_len, int32_t dtype, int32_t device, sgx_mdct **out) {
    if (out) *out = nullptr;
    if (!out) return fail<sgx_mdct>(nullptr, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::string msg;
    const sgx_status vs = validate(window_size, hop_size, window_kind, custom_window, custom_window_len, dtype, msg);
    if (vs != SGX_OK) return fail<sgx_mdct>(nullptr, vs, msg);
    sgx_mdct *p = new (std::nothrow) sgx_mdct();
    if (!p) return fail<sgx_mdct>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->two_n = window_size; p->n = window_size / 2; p->hop = hop_size;
    p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    p->window_kind = window_kind; p->window_param = window_param;
    if (window_kind == SGX_WIN_CUSTOM) p->custom.assign(custom_window, custom_window + custom_window_len);
    sgx_params wp{};
    wp.n_fft = uint32_t(window_size);
    wp.window_kind = window_kind;
    wp.window_param = window_param;
    make_window_f64(wp, p->custom, p->window);
    const size_t N = p->n, M = N / 2;
    unsigned fa, fb, fc;
#ifdef SGX_MDCT_NO_FUSED  // A/B builds only (tools/time_mdct.py): every shape on the generic route
    p->fused_fwd = false;
#else
    p->fused_fwd = N % 2 == 0 && fused_frame_bytes(unsigned(M), dtype, &fa, &fb, &fc) != 0 && fused_ltile(unsigned(M), dtype, 0, false) >= 0;
    // k_mdct_fwd indexes a tile's samples in 32 bits (so + i, so = s hop, s <= 31, i < 2N): a hop past that takes the generic fold,
    // whose f hop is 64-bit
    if (31ull * hop_size + window_size > (1ull << 32)) p->fused_fwd = false;
#endif
    p->fused_inv = p->fused_fwd && hop_size == N && fused_ltile(unsigned(M), dtype, 0, true) >= 2;
    p->L = unsigned(N % 2 == 0 ? M : N);
    if (device == -2) { *out = p; return SGX_OK; }  // host-only: validation, shapes, window, routes

    auto tables = [&]() -> sgx_status {
        if (device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        sgx_status st;
        if ((st = upload(p, p->d_win, p->window, dtype)) != SGX_OK) return st;
        const double n = double(N);
        if (N % 2 == 0) {
            if ((st = upload(p, p->d_t1, ctab(M, 1.0, [&](double k) { return -kPiM * (4.0 * k + 1.0) / (4.0 * n); }), dtype)) != SGX_OK) return st;
            if ((st = upload(p, p->d_t2, ctab(M, 1.0, [&](double k) { return -kPiM * k / n; }), dtype)) != SGX_OK) return st;
            if ((st = upload(p, p->d_t2i, ctab(M, 2.0 / n, [&](double k) { return -kPiM * k / n; }), dtype)) != SGX_OK) return st;
            if ((st = upload(p, p->d_tw, ctab(M, 1.0, [&](double k) { return -2.0 * kPiM * k / double(M); }), dtype)) != SGX_OK) return st;
        } else {
            if ((st = upload(p, p->d_pa, ctab(2 * N, 1.0, [&](double k) { return -kPiM * k / (2.0 * n); }), dtype)) != SGX_OK) return st;
            if ((st = upload(p, p->d_pb, ctab(N, 1.0, [&](double k) { return -kPiM * k / n; }), dtype)) != SGX_OK) return st;
            // (the product (1 + N)(2k + 1) reduced mod 8N in integers first: the angle itself reaches N pi / 2)
            if ((st = upload(p, p->d_phi, ctab(N, 1.0, [&](double k) {
                     const unsigned long long r = (unsigned long long)(N + 1) * (2ull * (unsigned long long)k + 1ull) % (8ull * N);
                     return -kPiM * double(r) / (4.0 * n);
                 }), dtype)) != SGX_OK)
                return st;
            const double off = double((N + 1) / 2);
            if ((st = upload(p, p->d_psi, ctab(2 * N, 2.0 / n, [&](double m) { return -kPiM * (m + off) / (2.0 * n); }), dtype)) != SGX_OK) return st;
            if ((st = upload(p, p->d_twL, ctab(N, 1.0, [&](double k) { return -2.0 * kPiM * k / n; }), dtype)) != SGX_OK) return st;
        }
        // generic route: chirp-z tables for a transform length without a pass split (as fft2d.hip's c2c_dispatch)
        const unsigned L = p->L;
        BsHostTables h;
        if (L >= 16 && (L & (L - 1)) != 0 && !reg_split_len(L, dtype, &fa, &fb, &fc) && bluestein_host_tables(L, dtype, h)) {
            if ((st = upload_bs(p, p->bs, h, dtype)) != SGX_OK) return st;
        }
        if (L >= 16 && !reg_split_len(L, dtype, &fa, &fb, &fc) && !p->bs.M && fft2d_tile_for(L, dtype) == 0)
            return fail(p, SGX_BACKEND, "hip -- FFT backend error: no complex transform kernel for length " + std::to_string(L));
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_mdct_destroy);
}

void sgx_mdct_destroy(sgx_mdct *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    bs_free(p->bs);
    delete p;
}

sgx_status sgx_mdct_output_shape(const sgx_mdct *p, size_t n_samples, size_t *n_coeffs, size_t *n_frames) {
    if (!p || !n_coeffs || !n_frames) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (n_samples < p->two_n)
        return fail(p, SGX_INVALID_INPUT, "Invalid input: samples length (" + std::to_string(n_samples) + ") must be >= window_size (" +
                                               std::to_string(p->two_n) + ")");  // src/mdct.rs:398-404
    *n_coeffs = p->n;
    *n_frames = frames_of(p, n_samples);
    return SGX_OK;
}

sgx_status sgx_mdct_inverse_length(const sgx_mdct *p, size_t n_frames, size_t *n_samples) {
    if (!p || !n_samples) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    *n_samples = inv_len(p, n_frames);
    return SGX_OK;
}

sgx_status sgx_mdct_forward(sgx_mdct *p, const void *samples, size_t batch, size_t n_samples, void *out, size_t out_elems, int32_t mem_kind,
                            void *hip_stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (!samples || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    size_t nc, nf;
    sgx_status st = sgx_mdct_output_shape(p, n_samples, &nc, &nf);
    if (st != SGX_OK) return st;
    if (batch > 0xffffffffull || nf > 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or frame count too large");
    const size_t expected = batch * nc * nf;
    if (out_elems != expected)
        return dim_mismatch(p, expected, out_elems);
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return with_staging(p, samples, batch * n_samples * p->elem, out, expected * p->elem, mem_kind, s,
                        [&](const void *i, void *o) { return run_dev(p, i, batch, n_samples, nf, o, false, s); });
}

sgx_status sgx_mdct_inverse(sgx_mdct *p, const void *coeffs, size_t batch, size_t n_coeffs, size_t n_frames, void *out, size_t out_elems,
                            int32_t mem_kind, void *hip_stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (n_coeffs != p->n)  // src/mdct.rs:451-457
        return dim_mismatch(p, p->n, n_coeffs,
                            " (coefficients has " + std::to_string(n_coeffs) + " rows but params.n_coefficients() = " + std::to_string(p->n) + ")");
    if (batch > 0xffffffffull || n_frames > 0x7fffffffull) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or frame count too large");
    const size_t len = inv_len(p, n_frames), expected = batch * len;
    if (out_elems != expected)
        return dim_mismatch(p, expected, out_elems);
    if (n_frames == 0) return SGX_OK;  // zero frames: an empty output (src/mdct.rs:459-462)
    if (!coeffs || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return with_staging(p, coeffs, batch * n_coeffs * n_frames * p->elem, out, expected * p->elem, mem_kind, s,
                        [&](const void *i, void *o) { return run_dev(p, i, batch, 0, n_frames, o, true, s); });
}

sgx_status sgx_mdct_reserve(sgx_mdct *p, size_t batch, size_t n_samples, int32_t host_staging) {
    if (!p || batch == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: batch must be > 0");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    size_t nc, nf;
    sgx_status st = sgx_mdct_output_shape(p, n_samples, &nc, &nf);
    if (st != SGX_OK) return st;
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (!p->fused_fwd && (st = gen_reserve(p, batch * nf, false)) != SGX_OK) return st;
    if (!p->fused_inv && (st = gen_reserve(p, batch * nf, true)) != SGX_OK) return st;
    if (host_staging) {
        const size_t big = std::max(batch * n_samples, std::max(batch * nc * nf, batch * inv_len(p, nf))) * p->elem;
        if ((st = grow(p, p->d_in, big)) != SGX_OK) return st;
        if ((st = grow(p, p->d_out, big)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_mdct_window(const sgx_mdct *p, double *out) {
    if (!p || !out) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    std::memcpy(out, p->window.data(), p->window.size() * sizeof(double));
    return SGX_OK;
}

const char *sgx_mdct_kernel_name(const sgx_mdct *p, int32_t inverse) {
    if (!p) return "";
    if (inverse) return p->fused_inv ? "k_imdct_ola" : "imdct_generic";
    return p->fused_fwd ? "k_mdct_fwd" : "mdct_generic";
}

int32_t sgx_mdct_device(const sgx_mdct *p) { return p ? p->device : -2; }

const char *sgx_mdct_last_error(const sgx_mdct *p) { return p ? p->err.c_str() : create_err<sgx_mdct>().c_str(); }

}  // extern "C"

namespace {

sgx_status with_staging(sgx_mdct *p, const void *in, size_t in_bytes, void *out, size_t out_bytes, int mem_kind, hipStream_t s,
                        const std::function<sgx_status(const void *, void *)> &body) {
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return body(in, out);
    if (mem_kind != SGX_MEM_HOST) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    sgx_status st;
    if ((st = grow(p, p->d_in, in_bytes)) != SGX_OK) return st;
    if ((st = grow(p, p->d_out, out_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, in, in_bytes, hipMemcpyHostToDevice, s));
    if ((st = body(p->d_in, p->d_out)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

}  // namespace

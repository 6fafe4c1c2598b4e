// cqt.hip — constant-Q spectrogram frames (MappingKind::Cqt, src/spectrogram.rs:1882-1904 over CqtKernel::apply, src/cqt.rs:495-522)
// on the matrix cores.
//
// Every bin is a time-domain correlation of the frame's last L_k samples with one complex kernel, so a batch of frames against all
// bins is a GEMM: rows = frames, K = taps, columns = (Re, -Im) of each bin's kernel.  The host (plan.hip cqt_device_tables) packs the
// bins in groups of 8 (16 columns) as dense [L_g][16] blocks right-aligned at the frame's end (sgx_internal.h CqtArgs), so group g
// only runs the taps [n_fft - L_g, n_fft): the short kernels of the high bins skip the early taps with a wave-uniform loop bound.
//
//   k_cqt<T, M, LDS>: one 256-thread workgroup per tile of F = 16 M consecutive frames of one signal.  The tile's sample span
//   ((F - 1) hop + lpad samples) is copied to LDS once (LDS = true; zero outside the signal, the centre padding of S1), then each of
//   the 4 waves runs its share of the groups (balanced on the host): per 4-tap step one B fragment (the group block, L2-resident) and
//   M A fragments (16 frames each, from LDS) into M accumulators of v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 — both a k-ordered
//   fma chain in T.  LDS = false reads the A operands from global memory (spans too large for LDS: long hops, f64 long kernels).
//   Epilogue: Re / Im meet across the lane pair (2c, 2c + 1), |Y|^2 = re re + im im in T (Complex::norm_sqr), then the amplitude
//   scale, stored [b][bin][frame].  CPLX = true (the transform plans' complex output, cqt() of src/cqt.rs:656-709) stores (re, im)
//   itself, one complex value per store.
//   ROWS = true (transform plans, one frame per signal): the 16 M rows of a tile are 16 M consecutive signals instead of 16 M frames of
//   one signal — the A row pitch is the sample stride and the A operands come from global memory.  Each output is the same k-ordered
//   fma chain over the same taps as on the per-signal tiles, so the two routes give the same bits.
//
// Non-finite samples.  Inside a group a shorter bin has zero weights in front of its own L_k taps; 0 x NaN = NaN would let a NaN /
// Inf that the reference never multiplies for that bin poison it.  The span copy marks every frame that has a non-finite sample
// anywhere in its [n_fft - lpad, n_fft) reach; the GEMM epilogue skips those frames and they are recomputed exactly — each bin over its
// own L_k taps, sequential accumulation of T(coefficient) * x with separate roundings, as the reference does — at the end of the tile.
//
// LDS bank skew: the A fragment of a step reads 16 frame rows hop words apart; for hops that are a multiple of 8 words those rows fall
// on 2 .. 16 banks only.  The copy then inserts one word after every hop words of the span: row r of the fragment starts at
// r (hop + 1) + t + floor(t / hop) for tap offset t, an odd row pitch that spreads the 16 rows over 16 banks.
#include <hip/hip_runtime.h>

#include "db_f64.h"
#include "sgx_internal.h"

namespace sgx {
namespace {

template <typename T>
struct Mf;
template <>
struct Mf<float> {
    typedef float V4 __attribute__((ext_vector_type(4)));
    typedef float V2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ V4 mfma(float a, float b, V4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    // C/D: lane l, register e holds row 4 (l >> 4) + e, column l & 15
    static __device__ __forceinline__ unsigned row(unsigned l, unsigned e) { return 4u * (l >> 4) + e; }
};
template <>
struct Mf<double> {
    typedef double V4 __attribute__((ext_vector_type(4)));
    typedef double V2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ V4 mfma(double a, double b, V4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    // the f64 form does not use the f32 map (cdna_hip_programming.md §3): row (l >> 4) + 4 e, column l & 15
    static __device__ __forceinline__ unsigned row(unsigned l, unsigned e) { return (l >> 4) + 4u * e; }
};

__device__ __forceinline__ bool finite_t(float v) { return __builtin_isfinite(v); }
__device__ __forceinline__ bool finite_t(double v) { return __builtin_isfinite(v); }
// the reference's `acc += T::from_f64(c) * x` and `re * re + im * im` are separate roundings (rustc never contracts).  __fmul_rn /
// __dmul_rn / __fadd_rn / __dadd_rn are plain `*` and `+` in the HIP headers, which hipcc's default -ffp-contract=fast-honor-pragmas
// fuses (it did in every f64 instance: v_mul_f64 + v_fmac_f64); only the pragma keeps the two roundings apart.
template <typename T>
__device__ __forceinline__ T mul_rn(T a, T b) {
#pragma clang fp contract(off)
    return a * b;
}
template <typename T>
__device__ __forceinline__ T add_rn(T a, T b) {
#pragma clang fp contract(off)
    return a + b;
}

// f64 only: hold every consumer of the accumulators back until the last v_mfma_f64_16x16x4_f64 of a 16-tap step has retired.  The
// instruction takes 16 passes on gfx950; the wait states hipcc puts in front of the v_accvgpr_read of its result (11) are those of
// an 8-pass instruction.  In the M = 1 instances the accumulator goes through VGPRs once per step, and without the LDS skew nothing
// else stands between the 4th MFMA and that read: the last register written, the high word of element 3 (frame rows 12 .. 15), was
// read before the MFMA wrote it, so those rows lost every 4th MFMA (tests/test_cqt_readback.py, hop 441 f64).  64 wait states on
// top of the compiler's own are what the whole suite ran with (13 % at the f64 bench shape); 32 passed the read-back as well, and
// 16, one per pass, should suffice but has not run.
#define SGX_CQT_DRAIN_ASM "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15"
template <int M>
__device__ __forceinline__ void mfma_drain(Mf<float>::V4 (&)[M]) {}
template <int M>
__device__ __forceinline__ void mfma_drain(Mf<double>::V4 (&acc)[M]) {
    static_assert(M == 1 || M == 2 || M == 4, "one operand list per tile multiple");
    if constexpr (M == 1) asm volatile(SGX_CQT_DRAIN_ASM : "+a"(acc[0]));
    if constexpr (M == 2) asm volatile(SGX_CQT_DRAIN_ASM : "+a"(acc[0]), "+a"(acc[1]));
    if constexpr (M == 4) asm volatile(SGX_CQT_DRAIN_ASM : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]));
}
#undef SGX_CQT_DRAIN_ASM

// amplitude scale of a power value (src/spectrogram.rs:1986-2080): sqrt, or 10 log10(max(p, eps)) — max ignores a NaN power like
// f32::max / f64::max; f32 dB through the hardware log2 as the other kernels, f64 through db_f64.h
__device__ __forceinline__ float amp_t(float p, int amp, float eps) {
    if (amp == AMP_MAGNITUDE) return sqrtf(p);
    if (amp == AMP_DB) return __builtin_log2f(fmaxf(p, eps)) * 3.01029995663981195f;
    return p;
}
__device__ __forceinline__ double amp_t(double p, int amp, double eps) {
    if (amp == AMP_MAGNITUDE) return sqrt(p);
    if (amp == AMP_DB) return db_f64(fmax(p, eps));
    return p;
}

template <typename T>
__device__ __forceinline__ T sample_at(const T *xb, long long s, unsigned long long n) {
    return (s >= 0 && (unsigned long long)s < n) ? xb[s] : T(0);
}

// one output value: (re, im) as one store of 2 T (rows are only 2 T aligned), or the amplitude of |Y|^2
template <typename T, bool CPLX>
__device__ __forceinline__ void put_bin(T *out, size_t at, T re, T im, int amp, T eps) {
    if (CPLX) {
        typedef typename Mf<T>::V2 V2;
        reinterpret_cast<V2 *>(out)[at] = V2{re, im};
    } else {
        const T pw = add_rn(mul_rn(re, re), mul_rn(im, im));
        out[at] = amp_t(pw, amp, eps);
    }
}

template <typename T, int M, bool LDS, bool CPLX, bool ROWS>
__global__ __launch_bounds__(256) void k_cqt(CqtArgs a) {
    static_assert(!(ROWS && LDS), "the spans of 16 M signals do not fit LDS");
    typedef typename Mf<T>::V4 V4;
    constexpr unsigned F = 16u * M;
    extern __shared__ unsigned char smem[];
    __shared__ unsigned long long s_bad;  // frames of the tile with a non-finite sample in reach (bit r: frame f0 + r)
    T *span_lds = reinterpret_cast<T *>(smem);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // ROWS: b is the tile's first signal and every row is frame 0 of signal b + row
    const unsigned b = ROWS ? blockIdx.x * F : blockIdx.x / a.tiles, f0 = ROWS ? 0u : (blockIdx.x % a.tiles) * F;
    const T *xb = static_cast<const T *>(a.x) + (size_t)b * a.sample_stride;
    const unsigned hop = a.hop, lpad = a.lpad;
    const unsigned skew = (hop % 8u == 0u) ? 1u : 0u;
    // signal index of span offset 0: frame f0's tap n_fft - lpad
    const long long s0 = (long long)f0 * hop - (long long)a.pad + (long long)a.n_fft - (long long)lpad;
    const unsigned span = (F - 1u) * hop + lpad;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (ROWS) {  // per row: that signal's [n_fft - lpad, n_fft) reach
        for (unsigned p = tid; p < F * lpad; p += 256u) {
            const unsigned r = p / lpad;
            if ((unsigned long long)b + r >= a.batch) break;
            const T v = sample_at(xb + (size_t)r * a.sample_stride, s0 + (long long)(p - r * lpad), a.n_samples);
            if (!finite_t(v)) atomicOr(&s_bad, 1ull << r);
        }
    }
    for (unsigned p = tid; !ROWS && p < span; p += 256u) {
        const T v = sample_at(xb, s0 + (long long)p, a.n_samples);
        if (LDS) span_lds[p + (skew ? p / hop : 0u)] = v;
        if (!finite_t(v)) {  // frames r with r hop <= p < r hop + lpad
            const unsigned rlo = p >= lpad ? (p - lpad) / hop + 1u : 0u;
            const unsigned rhi = min(p / hop, F - 1u);
            unsigned long long m = 0;
            for (unsigned r = rlo; r <= rhi; ++r) m |= 1ull << r;
            if (m) atomicOr(&s_bad, m);
        }
    }
    __syncthreads();
    const unsigned long long bad = s_bad;

    const T *tab = static_cast<const T *>(a.tab);
    const unsigned *info = a.info;
    const unsigned *wave_begin = info + 4u * a.n_groups;
    const unsigned *order = wave_begin + kCqtWaves + 1u;
    T *out = static_cast<T *>(a.out);
    const T eps = T(a.eps);
    const unsigned rr = lane & 15u, kq = lane >> 4;
    const unsigned row_pitch = hop + skew;  // LDS words between frame rows
    for (unsigned gi = wave_begin[wave]; gi < wave_begin[wave + 1u]; ++gi) {
        const unsigned g = order[gi];
        const unsigned off = info[4u * g], Lg = info[4u * g + 1u], bin0 = info[4u * g + 2u];
        // B fragment of step s: rows 4 s + kq of the block, column rr
        const T *bp = tab + ((size_t)off + kq) * 16u + rr;
        unsigned t = lpad - Lg + kq;  // this lane's tap offset within the span row
        unsigned q = 0, rem = t;      // t = q hop + rem (skewed addressing)
        if (skew) { q = t / hop; rem = t - q * hop; }
        unsigned addr = rr * row_pitch + t + q;  // LDS word of (frame rr, tap t)
        long long gaddr = s0 + (long long)rr * hop + t;  // signal index of the same (global A path)
        if (ROWS) gaddr = s0 + (long long)t;
        const T *xrow[M];  // ROWS: the signals of this lane's A rows (rr + 16 i), null past the batch
        if (ROWS) {
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const unsigned long long sig = (unsigned long long)b + rr + 16u * (unsigned)i;
                xrow[i] = sig < a.batch ? xb + (size_t)(rr + 16u * (unsigned)i) * a.sample_stride : nullptr;
            }
        }
        V4 acc[M];
#pragma unroll
        for (int i = 0; i < M; ++i) acc[i] = V4{0, 0, 0, 0};
        T bn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bn[u] = bp[u * 64];
        for (unsigned j = 0; j < Lg; j += 16u) {
            T bc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) bc[u] = bn[u];
            if (j + 16u < Lg) {
#pragma unroll
                for (int u = 0; u < 4; ++u) bn[u] = bp[(size_t)(j + 16u) * 16u + u * 64];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    T av;
                    if (LDS) av = span_lds[addr + (unsigned)i * 16u * row_pitch];
                    else if (ROWS) av = xrow[i] ? sample_at(xrow[i], gaddr, a.n_samples) : T(0);
                    else av = sample_at(xb, gaddr + (long long)i * 16 * hop, a.n_samples);
                    acc[i] = Mf<T>::mfma(av, bc[u], acc[i]);
                }
                addr += 4u;
                gaddr += 4;
                if (skew) {
                    rem += 4u;
                    if (rem >= hop) { rem -= hop; addr += 1u; }
                }
            }
            mfma_drain<M>(acc);
        }
        // epilogue: column rr = 2 c + (0: Re, 1: Im) of bin bin0 + c; lanes rr and rr ^ 1 hold the two parts of the same rows
        const unsigned bin = bin0 + (rr >> 1);
        const bool odd = (rr & 1u) != 0u;
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (unsigned e = 0; e < 4u; ++e) {
                const T v = acc[i][e];
                const T w = __shfl_xor(v, 1);
                const T re = odd ? w : v, im = odd ? v : w;
                const unsigned fr = 16u * i + Mf<T>::row(lane, e), frame = ROWS ? 0u : f0 + fr;
                const bool live = ROWS ? (unsigned long long)b + fr < a.batch : frame < a.n_frames;
                // the pair splits the stores: the Re lane takes registers 0, 1, the Im lane 2, 3
                if ((e >> 1) == (odd ? 1u : 0u) && bin < a.n_bins && live && !((bad >> fr) & 1ull))
                    put_bin<T, CPLX>(out, ((size_t)b * a.n_bins + (ROWS ? (size_t)fr * a.n_bins : 0) + bin) * a.n_frames + frame, re, im,
                                     a.amp, eps);
            }
        }
    }

    // exact recompute of the frames with a non-finite sample in reach (rare: a wave-uniform skip otherwise)
    if (bad) {
        for (unsigned fr = 0; fr < F; ++fr) {
            const unsigned frame = ROWS ? 0u : f0 + fr;
            if (!((bad >> fr) & 1ull) || frame >= a.n_frames) continue;  // (ROWS: only rows inside the batch are ever marked)
            const T *xs = ROWS ? xb + (size_t)fr * a.sample_stride : xb;
            for (unsigned k = tid; k < a.n_bins; k += 256u) {
                const unsigned g = k >> 3, c = k & 7u;
                const unsigned off = info[4u * g], Lg = info[4u * g + 1u], Lk = a.len[k];
                const T *col = tab + (size_t)off * 16u + 2u * c;
                // signal index of block row 0 = frame tap n_fft - Lg; the bin's own taps are rows Lg - Lk .. Lg - 1
                const long long sb = (long long)frame * hop - (long long)a.pad + (long long)a.n_fft - (long long)Lg;
                T re = T(0), im = T(0);
                for (unsigned jr = Lg - Lk; jr < Lg; ++jr) {
                    const T xv = sample_at(xs, sb + (long long)jr, a.n_samples);
                    re = add_rn(re, mul_rn(col[(size_t)jr * 16u], xv));
                    im = add_rn(im, mul_rn(col[(size_t)jr * 16u + 1u], xv));
                }
                put_bin<T, CPLX>(out, ((size_t)b * a.n_bins + (ROWS ? (size_t)fr * a.n_bins : 0) + k) * a.n_frames + frame, re, im, a.amp, eps);
            }
        }
    }
}

// Rows route: 16 signals per workgroup.  A wider tile would reuse each B fragment for more rows, but it also divides the number of
// workgroups, and at 16 signals a batch of 4096 is one workgroup per CU; the group blocks it re-reads stay in L2.
constexpr int kCqtRowsM = 1;
constexpr size_t kCqtLdsMax = 160u * 1024u - 64u;  // dynamic LDS of one workgroup (s_bad is static)
#ifndef SGX_CQT_LDS_PREF
#define SGX_CQT_LDS_PREF (80u * 1024u - 64u)  // spans up to this size leave room for two workgroups per CU
#endif

size_t cqt_lds_bytes(unsigned m, unsigned hop, unsigned lpad, size_t elem) {
    const size_t span = size_t(16u * m - 1u) * hop + lpad;
    const size_t words = span + ((hop % 8u == 0u) ? span / hop + 1u : 0u);
    return words * elem;
}

template <typename T, int M, bool LDS, bool CPLX, bool ROWS>
hipError_t launch_t(const CqtArgs &a, hipStream_t s) {
    const size_t lds = LDS ? cqt_lds_bytes(M, a.hop, a.lpad, sizeof(T)) : 0;
    if (lds > 64u * 1024u) {
        const hipError_t e = set_max_dynamic_lds((const void *)k_cqt<T, M, LDS, CPLX, ROWS>, (int)kCqtLdsMax);
        if (e != hipSuccess) return e;
    }
    const unsigned long long blocks = ROWS ? ((unsigned long long)a.batch + 16u * M - 1u) / (16u * M) : (unsigned long long)a.batch * a.tiles;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((k_cqt<T, M, LDS, CPLX, ROWS>), dim3((unsigned)blocks), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <typename T, bool CPLX>
hipError_t launch_dt(const CqtArgs &a, unsigned m, bool rows, hipStream_t s) {
    if (rows) return launch_t<T, kCqtRowsM, false, CPLX, true>(a, s);
    switch (m) {
    case 4: return launch_t<T, 4, true, CPLX, false>(a, s);
    case 2: return launch_t<T, 2, true, CPLX, false>(a, s);
    case 1: return launch_t<T, 1, true, CPLX, false>(a, s);
    default: return launch_t<T, 4, false, CPLX, false>(a, s);
    }
}

}  // namespace

unsigned cqt_lds_m(unsigned hop, unsigned lpad, int dtype) {
    const size_t elem = dtype == SGX_F64 ? 8 : 4;
    for (size_t cap : {size_t(SGX_CQT_LDS_PREF), kCqtLdsMax})
        for (unsigned m : {4u, 2u, 1u})
            if (cqt_lds_bytes(m, hop, lpad, elem) <= cap) return m;
    return 0;
}

hipError_t launch_cqt(const CqtArgs &a0, unsigned lds_m, int dtype, bool cplx, bool rows, hipStream_t s) {
    CqtArgs a = a0;
    const unsigned F = 16u * (lds_m ? lds_m : 4u);
    a.tiles = (a.n_frames + F - 1u) / F;
    if (rows && a.n_frames != 1u) return hipErrorInvalidValue;  // (a row of the rows route is one signal's only frame)
    if (dtype == SGX_F64) return cplx ? launch_dt<double, true>(a, lds_m, rows, s) : launch_dt<double, false>(a, lds_m, rows, s);
    return cplx ? launch_dt<float, true>(a, lds_m, rows, s) : launch_dt<float, false>(a, lds_m, rows, s);
}

}  // namespace sgx

// rr_passes.h — the passes of the in-LDS transform on RrLayout tiles (rr_layout.h), once, for every kernel that runs a length
// N = A B C transform as two or three in-register passes around LDS exchanges (device code only).
//
// A sequence's tile is `seq = buf + s * RrLayout::FS`.  The per-item helpers (rr_pass1_store, rr_pass1_load, rr_last_load) take
// the work item's registers by reference and leave the code generation of their users as it was (k_welch keeps its pass 1: the
// note there).  The loop-level rr_pass2 / rr_pass3 do not: in k_c2c_reg, k_c2r_reg, k_welch, k_kaldi and bs_middle they move the
// register allocation across an occupancy step (profiles/rr_passes_codegen.txt), so those keep the same loops written out,
// each with a note, and the MDCT kernels, which have always run them as a helper, are their users.  No per-item helper holds a
// barrier; rr_passes23 has the three of mdct.hip's former mdct_passes23.
//
// Two differences between the users are intended and chosen per call site:
//   TABLE  every pass-1 twiddle W^(k1 r) is read from the table (one rounding) instead of being built by rr_twiddle from the
//          log2 entries W^(2^j r) (up to log2 - 1 products of entries): f64 k_kaldi (k_welch's own passes do the same in f64).
//   wrap   rr_wrap<N> is `& (N - 1)` for a power of two and `% N` otherwise; only the 2-D and MDCT kernels have mixed-radix N.
// TS is the stride of W_N in the table: tw holds W_(TS N)^k, k < TS N (k_c2r_reg shares the 2 N-entry table of its Hermitian fold).
#pragma once
#include "fft_inreg.h"
#include "reg_radix.h"
#include "rr_layout.h"

namespace sgx {

template <unsigned N>
__device__ __forceinline__ constexpr unsigned rr_wrap(unsigned e) { return ct_is_pow2(N) ? (e & (N - 1)) : (e % N); }

// points of the last pass (pass 3, or pass 2 of a two-pass split)
template <int B, int C>
constexpr unsigned rr_last_len() { return C > 1 ? C : B; }

// Pass 1 of work item r (< B C) of a sequence: A-point transform of v[n1] = z[B C n1 + r], times W_N^(k1 r), to row k1, position r.
template <typename T, int A_, int B_, int C_, bool TABLE = false, unsigned TS = 1>
__device__ __forceinline__ void rr_pass1_store(typename PairOf<T>::type (&v)[A_], typename PairOf<T>::type *seq, unsigned r,
                                               const typename PairOf<T>::type *tw) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, C = C_, N = A_ * B_ * C_;
    constexpr int LA = ct_log2_ceil(A);
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned RS = L::RS;
    inreg::MixFft<A, V>::run(v);
    const unsigned pp = L::hi_part(r / C) ^ (r % C);
    if constexpr (TABLE) {
        seq[pp ^ L::k1_mask(0)] = v[0];
#pragma unroll
        for (unsigned k1 = 1; k1 < A; ++k1) (seq + (pp ^ L::k1_mask(k1)))[k1 * RS] = inreg::cmulv(v[k1], tw[rr_wrap<TS * N>(TS * k1 * r)]);
    } else {
        V pw2[LA];
#pragma unroll
        for (int j = 0; j < LA; ++j) pw2[j] = tw[rr_wrap<TS * N>((TS << j) * r)];
        seq[pp ^ L::k1_mask(0)] = v[0];
#pragma unroll
        for (unsigned k1 = 1; k1 < A; ++k1) (seq + (pp ^ L::k1_mask(k1)))[k1 * RS] = inreg::cmulv(v[k1], rr_twiddle<LA>(pw2, k1));
    }
}

// The inverse of pass 1 (on conjugated data): gather row k1, position r, times W_N^(k1 r), A-point transform; v[n1] is point B C n1 + r.
template <typename T, int A_, int B_, int C_>
__device__ __forceinline__ void rr_pass1_load(typename PairOf<T>::type (&v)[A_], const typename PairOf<T>::type *seq, unsigned r,
                                              const typename PairOf<T>::type *tw) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, C = C_, N = A_ * B_ * C_;
    constexpr int LA = ct_log2_ceil(A);
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned RS = L::RS;
    V pw2[LA];
#pragma unroll
    for (int j = 0; j < LA; ++j) pw2[j] = tw[rr_wrap<N>((1u << j) * r)];
    const unsigned pp = L::hi_part(r / C) ^ (r % C);
    v[0] = seq[pp ^ L::k1_mask(0)];
#pragma unroll
    for (unsigned k1 = 1; k1 < A; ++k1) v[k1] = inreg::cmulv((seq + (pp ^ L::k1_mask(k1)))[k1 * RS], rr_twiddle<LA>(pw2, k1));
    inreg::MixFft<A, V>::run(v);
}

// Pass 2 in place on `nseq` sequences: work item (s, k1, n3) transforms the B points of row k1 at lo = n3; three-pass splits then
// multiply by W_(B C)^(k2 n3) = W_N^(A k2 n3).
template <typename T, int A_, int B_, int C_>
__device__ __forceinline__ void rr_pass2(typename PairOf<T>::type *buf, unsigned nseq, unsigned tid, const typename PairOf<T>::type *tw) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, B = B_, C = C_, N = A * B * C;
    constexpr int LB = ct_log2_ceil(B);
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned RS = L::RS, FS = L::FS;
    for (unsigned idx = tid; idx < nseq * A * C; idx += 256) {
        const unsigned s = idx / (A * C), q = idx % (A * C), k1 = q / C, n3 = q % C;
        V *row = buf + (size_t)s * FS + k1 * RS;
        const unsigned lp = n3 ^ L::k1_mask(k1);  // point n2 sits at lp ^ hi_part(n2)
        V x[B];
#pragma unroll
        for (unsigned n2 = 0; n2 < B; ++n2) x[n2] = row[lp ^ L::hi_part(n2)];
        inreg::MixFft<B, V>::run(x);
        row[lp ^ L::hi_part(0)] = x[0];
        if constexpr (C > 1) {
            V q2[LB];
#pragma unroll
            for (int j = 0; j < LB; ++j) q2[j] = tw[rr_wrap<N>((A << j) * n3)];
#pragma unroll
            for (unsigned k2 = 1; k2 < B; ++k2) row[lp ^ L::hi_part(k2)] = inreg::cmulv(x[k2], rr_twiddle<LB>(q2, k2));
        } else {
#pragma unroll
            for (unsigned k2 = 1; k2 < B; ++k2) row[lp ^ L::hi_part(k2)] = x[k2];
        }
    }
}

// Pass 3 in place on `nseq` sequences (three-pass splits): work item (s, k1, k2) transforms the C points at hi = k2.  Afterwards
// bin k1 + A (k2 + B k3) sits at RrLayout::of_output.
template <typename T, int A_, int B_, int C_>
__device__ __forceinline__ void rr_pass3(typename PairOf<T>::type *buf, unsigned nseq, unsigned tid) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, B = B_, C = C_;
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned RS = L::RS, FS = L::FS;
    for (unsigned idx = tid; idx < nseq * A * B; idx += 256) {
        const unsigned s = idx / (A * B), q = idx % (A * B), k1 = q / B, k2 = q % B;
        V *row = buf + (size_t)s * FS + k1 * RS;
        const unsigned lp = L::hi_part(k2) ^ L::k1_mask(k1);  // point n3 sits at lp ^ n3
        V x[C];
#pragma unroll
        for (unsigned n3 = 0; n3 < C; ++n3) x[n3] = row[lp ^ n3];
        inreg::MixFft<C, V>::run(x);
#pragma unroll
        for (unsigned k3 = 0; k3 < C; ++k3) row[lp ^ k3] = x[k3];
    }
}

// Passes 2 and 3 behind a pass 1 that wrote `nseq` sequences, with their barriers: the finished bins are visible on return.
template <typename T, int A_, int B_, int C_>
__device__ __forceinline__ void rr_passes23(typename PairOf<T>::type *buf, unsigned nseq, unsigned tid, const typename PairOf<T>::type *tw) {
    __syncthreads();
    rr_pass2<T, A_, B_, C_>(buf, nseq, tid, tw);
    __syncthreads();
    if constexpr (C_ > 1) {
        rr_pass3<T, A_, B_, C_>(buf, nseq, tid);
        __syncthreads();
    }
}

// The last pass into registers instead of in place: work item q of a sequence (q = k1 B + k2 < A B for three passes, q = k1 < A for
// two) ends with the bins k1 + A (k2 + B j), or k1 + A j, in vx[j], j < rr_last_len.  The caller forms the row pointer
// `row = seq + k1 * RS` and the lane part of the position, lp = (C > 1 ? hi_part(k2) : 0) ^ k1_mask(k1), from its own k1: with
// either formed in here the register allocation of k_kaldi<float, 16, 16, 8> moves (6 or 8 spilled registers against 4).
template <typename T, int A_, int B_, int C_>
__device__ __forceinline__ void rr_last_load(typename PairOf<T>::type (&vx)[(rr_last_len<B_, C_>())], const typename PairOf<T>::type *row, unsigned lp) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned C = C_, LAST = rr_last_len<B_, C_>();
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
#pragma unroll
    for (unsigned j = 0; j < LAST; ++j) vx[j] = row[lp ^ (C > 1 ? j : L::hi_part(j))];
    inreg::MixFft<LAST, V>::run(vx);
}

}  // namespace sgx

// bs_middle.h — the middle of an in-LDS circular convolution on the register-tiled passes, shared by the chirp-z kernels
// (bluestein.hip) and the overlap-save FIR kernel (fir.hip): forward passes 2 and 3, the product with a plan table taken where
// pass 3 leaves the bins, and the same passes run back (the derivation is at k_bs_fused).
// Its pass 2 shares a loop with the two-pass product and its back pass 2 is the only one of its kind, so both stay written out
// here instead of going through rr_pass2 (rr_passes.h): with rr_pass2 inside bs_middle k_fir_os<float, 16, 16, 8> went from 124
// to 146 registers (profiles/rr_passes_codegen.txt).  Pass 1 and its inverse around bs_middle are rr_pass1_store / rr_pass1_load.
#pragma once
#include "rr_passes.h"

namespace sgx {

#ifdef SGX_BS_STAMPS  // diagnostic build only (tools/stamps_bs.py): a wave's cycles per stage of k_bs_fused
#define BS_STAMP(i)                                                                \
    do {                                                                           \
        unsigned long long t_;                                                     \
        __builtin_amdgcn_sched_barrier(0);                                         \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                         \
        st_acc[i] += t_ - st_prev;                                                 \
        st_prev = t_;                                                              \
    } while (0)
#define BS_STAMP_PARAMS , unsigned long long *st_acc, unsigned long long &st_prev
#define BS_STAMP_ARGS , st_acc, st_prev
#else
#define BS_STAMP(i)
#define BS_STAMP_PARAMS
#define BS_STAMP_ARGS
#endif

// The middle of the convolution, shared by the frame kernel and the complex-sequence kernel: on entry every work item has written
// its P1 + T1 results to the tile; on return the tile holds conj(T1^-1-input of P1^-1), i.e. what P1^-1's work items read.
template <typename T, int A_, int B_, int C_>
__device__ __forceinline__ void bs_middle(typename PairOf<T>::type *buf, unsigned ns, unsigned tid, const typename PairOf<T>::type *tw,
                                          const typename PairOf<T>::type *bhp BS_STAMP_PARAMS) {
    typedef typename PairOf<T>::type V;
    constexpr unsigned A = A_, B = B_, C = C_, N = A * B * C;
    constexpr int LB = ct_log2_ceil(B);
    typedef RrLayout<sizeof(V), A_, B_, C_> L;
    constexpr unsigned RS = L::RS, FS = L::FS;
    __syncthreads();
    BS_STAMP(2);
    // P2 (+ T2); two-pass splits: P2, product, P2^-1
    for (unsigned idx = tid; idx < ns * A * C; idx += 256) {
        const unsigned s = idx / (A * C), q = idx % (A * C), k1 = q / C, n3 = q % C;
        V *row = buf + (size_t)s * FS + k1 * RS;
        const unsigned lp = n3 ^ L::k1_mask(k1);
        V v[B];
#pragma unroll
        for (unsigned n2 = 0; n2 < B; ++n2) v[n2] = row[lp ^ L::hi_part(n2)];
        inreg::MixFft<B, V>::run(v);
        if constexpr (C > 1) {
            V q2[LB];
#pragma unroll
            for (int j = 0; j < LB; ++j) q2[j] = tw[rr_wrap<N>((A << j) * n3)];
            row[lp ^ L::hi_part(0)] = v[0];
#pragma unroll
            for (unsigned k2 = 1; k2 < B; ++k2) row[lp ^ L::hi_part(k2)] = inreg::cmulv(v[k2], rr_twiddle<LB>(q2, k2));
        } else {
#pragma unroll
            for (unsigned k2 = 0; k2 < B; ++k2) {  // bin k1 + A k2; the table is [k2][k1]
                const V y = inreg::cmulv(v[k2], bhp[k2 * A + k1]);
                v[k2] = (V){y.x, -y.y};
            }
            inreg::MixFft<B, V>::run(v);
#pragma unroll
            for (unsigned n2 = 0; n2 < B; ++n2) row[lp ^ L::hi_part(n2)] = v[n2];
        }
    }
    BS_STAMP(3);
    __syncthreads();
    BS_STAMP(4);
    if constexpr (C > 1) {
        // P3, product, P3^-1 (from here on the data is the conjugate of the inverse transform's)
        for (unsigned idx = tid; idx < ns * A * B; idx += 256) {
            const unsigned s = idx / (A * B), q = idx % (A * B), k1 = q / B, k2 = q % B;
            V *row = buf + (size_t)s * FS + k1 * RS;
            const unsigned lp = L::hi_part(k2) ^ L::k1_mask(k1);
            V v[C], h[C];
#pragma unroll
            for (unsigned k3 = 0; k3 < C; ++k3) h[k3] = bhp[k3 * (A * B) + q];  // bin k1 + A (k2 + B k3); the table is [k3][k1][k2]
#pragma unroll
            for (unsigned n3 = 0; n3 < C; ++n3) v[n3] = row[lp ^ n3];
            inreg::MixFft<C, V>::run(v);
#pragma unroll
            for (unsigned k3 = 0; k3 < C; ++k3) {
                const V y = inreg::cmulv(v[k3], h[k3]);
                v[k3] = (V){y.x, -y.y};
            }
            inreg::MixFft<C, V>::run(v);
#pragma unroll
            for (unsigned n3 = 0; n3 < C; ++n3) row[lp ^ n3] = v[n3];
        }
        BS_STAMP(5);
        __syncthreads();
        BS_STAMP(6);
        // T2, P2
        for (unsigned idx = tid; idx < ns * A * C; idx += 256) {
            const unsigned s = idx / (A * C), q = idx % (A * C), k1 = q / C, n3 = q % C;
            V *row = buf + (size_t)s * FS + k1 * RS;
            const unsigned lp = n3 ^ L::k1_mask(k1);
            V q2[LB];
#pragma unroll
            for (int j = 0; j < LB; ++j) q2[j] = tw[rr_wrap<N>((A << j) * n3)];
            V v[B];
            v[0] = row[lp ^ L::hi_part(0)];
#pragma unroll
            for (unsigned k2 = 1; k2 < B; ++k2) v[k2] = inreg::cmulv(row[lp ^ L::hi_part(k2)], rr_twiddle<LB>(q2, k2));
            inreg::MixFft<B, V>::run(v);
#pragma unroll
            for (unsigned n2 = 0; n2 < B; ++n2) row[lp ^ L::hi_part(n2)] = v[n2];
        }
        BS_STAMP(7);
        __syncthreads();
        BS_STAMP(8);
    }
}

}  // namespace sgx

// binaural_kind.h — the kind functions of the binaural maps (src/binaural.rs), shared by the generic epilogue (binaural.hip) and the
// fused route of the tuned f32 n_fft 1024 kernel (kernels_r32x16.hip), so that both apply the same arithmetic to the same spectra.
// The kind codes are the SGX_BINAURAL_* values of spectro_hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include "spectro_hip.h"

namespace sgx {
namespace binaural {

// ---- the kind functions (src/binaural.rs), in T ---------------------------------------------------------------------------------
// Contraction is off in every body below: each product and sum is rounded on its own, as in the reference's Rust code (mul_add only
// where it says so).

template <typename T>
__device__ __forceinline__ T dev_sqrt(T x) { return sqrt(x); }
template <typename T>
__device__ __forceinline__ T dev_atan2(T y, T x) { return atan2(y, x); }
template <typename T>
__device__ __forceinline__ T dev_fmod(T x, T m) { return fmod(x, m); }
template <typename T>
__device__ __forceinline__ T dev_log10(T x) { return log10(x); }
template <typename T>
__device__ __forceinline__ T dev_fma(T a, T b, T c) { return fma(a, b, c); }

// magphase (:106-160): magnitude and the phase's angle.  mag_sq == 0 (underflow of tiny values included): mag 0, phase (1, 0), angle 0.
template <typename T>
struct MagPhase {
    T mag, mag_sq, re, im;  // re, im: the unit phase
};
template <typename T>
__device__ __forceinline__ MagPhase<T> magphase(T re, T im) {
#pragma clang fp contract(off)
    MagPhase<T> r;
    r.mag_sq = dev_fma(re, re, im * im);
    if (r.mag_sq == T(0)) {
        r.mag = T(0);
        r.re = T(1);
        r.im = T(0);
    } else {
        r.mag = dev_sqrt(r.mag_sq);
        const T inv = T(1) / r.mag;  // mag_val.recip()
        r.re = re * inv;
        r.im = im * inv;
    }
    return r;
}
template <typename T>
__device__ __forceinline__ T angle(const MagPhase<T> &m) { return dev_atan2(m.im, m.re); }

// pow_mag (:57-84) with mag = 0 kept at 0 (magphase writes 0 without calling it)
template <typename T>
__device__ __forceinline__ T pow_mag(const MagPhase<T> &m, unsigned power) {
#pragma clang fp contract(off)
    if (m.mag_sq == T(0)) return T(0);
    switch (power) {
        case 1: return m.mag;
        case 2: return m.mag_sq;
        case 3: return m.mag_sq * m.mag;
        case 4: return m.mag_sq * m.mag_sq;
        default: {
            T base = m.mag, acc = T(1);
            unsigned e = power;
            while (e > 0) {
                if (e & 1u) acc *= base;
                e >>= 1;
                if (e > 0) base *= base;
            }
            return acc;
        }
    }
}

template <typename T>
__device__ __forceinline__ T np_mod(T x, T m) {
#pragma clang fp contract(off)
    return dev_fmod(dev_fmod(x, m) + m, m);
}

template <typename T>
struct KindConst {
    T pi, two_pi, bw;  // T::PI, T(2) pi, T(bw)
    unsigned power;     // ITD magphase_power (>= 1)
    int wrapped;        // IPD
};

template <typename T, int KIND>
__device__ __forceinline__ T binaural_value(T lre, T lim, T rre, T rim, unsigned k, const KindConst<T> &c) {
#pragma clang fp contract(off)
    const MagPhase<T> L = magphase(lre, lim), R = magphase(rre, rim);
    if constexpr (KIND == SGX_BINAURAL_ITD) {
        const T intensity = pow_mag(L, c.power) + pow_mag(R, c.power);
        if (!(intensity > T(0))) return T(0);  // the map starts zeroed; a NaN intensity leaves the 0 as well
        const T wrapped = np_mod(angle(L) - angle(R) + c.pi, c.two_pi) - c.pi;
        return wrapped / (c.two_pi * c.bw * T(k));
    } else if constexpr (KIND == SGX_BINAURAL_IPD) {
        const T diff = angle(L) - angle(R);
        return c.wrapped ? np_mod(diff + c.pi, c.two_pi) - c.pi : diff;
    } else {
        const T l = L.mag, r = R.mag;
        if (!(l + r > T(0) && l > T(0) && r > T(0))) return T(NAN);
        if constexpr (KIND == SGX_BINAURAL_ILD) {
            return T(-20) * dev_log10(r / l);
        } else {
            const T ratio = r / l;
            return ratio < T(1) ? T(1) - ratio : -(T(1) - T(1) / ratio);
        }
    }
}

}  // namespace binaural
}  // namespace sgx

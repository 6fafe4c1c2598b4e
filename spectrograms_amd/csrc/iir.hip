// iir.hip — batched IIR filtering plans (sgx_iir_*) of libspectro_hip.so, kernels and host side: cascades of second-order sections
// along whole rows, after scipy.signal.sosfilt / sosfiltfilt (include/spectro_hip_iir.h).
//
// A section runs in Direct Form II transposed in f64, each product and sum rounded on its own:
//   y = b0 x + z0;   z0 = b1 x - a1 y + z1;   z1 = b2 x - a2 y
// With zero input the cascade's state z (2S values) moves linearly, z' = A z, and with M = A^L (L samples)
//   exit(block k) = exit_from_zero_state(block k) + M exit(block k - 1).
// k_iir_sos<T, S, BACK>: a workgroup of 256 work items takes a tile of 256 L consecutive samples of one row, widened to f64 in LDS (work
// item k owns samples k L .. k L + L - 1; its LDS row is L + 1 values long, so that the 32 work items of a lane group walk 32 different
// banks in f32 and all 64 in f64).  Pass 1 runs every block from zero state (block 0 from the tile's entry state); a log-step scan
// s_k += M^(2^j) s_(k - 2^j), j = 0 .. 7, over LDS turns the 256 exit states into the true ones; pass 2 runs every block again from its
// true entry state, in place in LDS, and the tile is stored coalesced as T.  The tables M^(2^j) come from the host, which runs the
// recurrence itself in long double on unit states (no products of rounded matrices).  BACK walks the row from its end (logical sample
// t is physical sample n - 1 - t); the odd extension of filtfilt is an index map in the load; a store window trims it.
//
// Modes of the one kernel (a launch argument):
//   0  whole rows: a workgroup walks the tiles of its row in order, the state stays in LDS ("k_iir_sos")
//   1  split, launch 1: a workgroup per (row, segment of kSegTiles tiles) from zero state; pass 1 and the scan only, the segment's exit
//      state goes to E
//   2  split, launch 3: a workgroup per (row, segment) from the entry state k_iir_link (launch 2) chained through M^(segment)
// No workgroup waits on another: the three launches are the only dependencies.  The chain route ("iir_chain") runs passes of at
// most 8 sections in mode 0 through f64 scratch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "plan_host.h"
#include "spectro_hip_iir.h"

using namespace sgx;

namespace {

typedef unsigned long long u64;

constexpr unsigned kL = 16, kTile = 256 * kL, kLevels = 8, kSegTiles = SGX_IIR_SEGMENT_TILES, kMaxS = 8;
constexpr u64 kSeg = u64(kSegTiles) * kTile;
constexpr size_t kSplitBelowRows = 128;  // "auto": fewer rows than this, each of at least two segments, take the split route

// the instances: sections per pass, declared once (a shorter cascade is padded with identity sections, which are exact)
#define SGX_IIR_SECTIONS(X) X(1) X(2) X(4) X(8)

struct IirArgs {
    const void *in;  // rows of T, or of f64 when in_wide
    void *out;       // likewise (out_wide)
    u64 in_stride, out_stride;
    u64 n;           // logical samples per row
    u64 n_in;        // samples of the input row when pad > 0 (n = n_in + 2 pad)
    u64 out_lo, out_n;  // physical samples [out_lo, out_lo + out_n) are stored, at out[p - out_lo]
    const double *sos;  // [rows or 1][ns][6] of this pass
    const double *M;    // [rows or 1][kLevels + 1][D][D] of this pass, D = 2 S of the instance; the last table is M^(segment)
    const double *zi;   // entry state [..][2 ns] (nullptr: zero)
    const double *scale;  // [rows]: the entry state is zi * scale[row] (nullptr: zi as it is)
    double *zf;           // final state [rows][..] (nullptr: not wanted)
    double *E;            // modes 1 and 2: [rows][nseg][D], exit states from zero state / entry states
    u64 sos_stride, m_stride, zi_stride, zf_stride;  // doubles between rows (0: shared)
    unsigned pad, ns, nseg, mode, in_wide, out_wide;
};

template <int S>
struct Coef {
    double b0[S], b1[S], b2[S], a1[S], a2[S];
};

// one sample through the cascade; every operation rounds on its own, in the order of the header's formula
template <int S>
__device__ __forceinline__ double iir_step(const Coef<S> &c, double (&z)[2 * S], double x) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const double y = c.b0[i] * x + z[2 * i];
        z[2 * i] = c.b1[i] * x - c.a1[i] * y + z[2 * i + 1];
        z[2 * i + 1] = c.b2[i] * x - c.a2[i] * y;
        x = y;
    }
    return x;
}

// sum + m v as the error-free pieces of the product and of the sum: the new sum, its error added to `err`
__device__ __forceinline__ double iir_acc2(double sum, double m, double v, double &err) {
#pragma clang fp contract(off)
    const double h = m * v, e = __builtin_fma(m, v, -h);
    const double s = sum + h, bb = s - sum;
    err += ((sum - (s - bb)) + (h - bb)) + e;
    return s;
}

// z += M nb, every row as one dot product carried in twice the working precision and rounded once.  A table's large entries cancel
// against each other when the poles lie close to the circle (|M| |s| is thousands of times |M s| for a high-pass at 0.001), and plain
// f64 products then cost several times the sequential recurrence's own error.  A section's state moves with the sections in front of
// it only: M is block lower triangular.
template <int S>
__device__ __forceinline__ void iir_link(const double *M, const double (&nb)[2 * S], double (&z)[2 * S]) {
    constexpr int D = 2 * S;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double sum = z[r], err = 0.0;
#pragma unroll
        for (int q = 0; q < 2 * (r / 2 + 1); ++q) sum = iir_acc2(sum, M[r * D + q], nb[q], err);
        z[r] = sum + err;
    }
}

template <typename T>
__device__ __forceinline__ double iir_at(const void *row, unsigned wide, u64 i) {
    return wide ? ((const double *)row)[i] : (double)((const T *)row)[i];
}

// physical sample p of the row: the samples themselves, or their odd extension by pad on both sides
template <typename T>
__device__ __forceinline__ double iir_load(const IirArgs &a, const void *row, u64 p) {
    if (a.pad == 0) return iir_at<T>(row, a.in_wide, p);
    if (p < a.pad) return 2.0 * iir_at<T>(row, a.in_wide, 0) - iir_at<T>(row, a.in_wide, a.pad - p);
    if (p >= a.pad + a.n_in) return 2.0 * iir_at<T>(row, a.in_wide, a.n_in - 1) - iir_at<T>(row, a.in_wide, a.n_in - 2 - (p - a.pad - a.n_in));
    return iir_at<T>(row, a.in_wide, p - a.pad);
}

template <typename T, int S, bool BACK>
__global__ __launch_bounds__(256) void k_iir_sos(IirArgs a) {
    constexpr int D = 2 * S;
    constexpr unsigned L = kL, LS = L + 1, TILE = 256 * L;
    extern __shared__ __attribute__((aligned(16))) double iir_smem[];
    double *tile = iir_smem;          // [256][L + 1]
    double *sc = iir_smem + 256 * LS;  // [D][256]: the scan's states, component-major
    __shared__ double ent[D];         // the tile's entry state
    const unsigned tid = threadIdx.x;
    const unsigned row = a.mode ? blockIdx.x / a.nseg : blockIdx.x, seg = a.mode ? blockIdx.x % a.nseg : 0;
    const u64 t_begin = a.mode ? seg * kSeg : 0;
    const u64 t_end = a.mode ? min(a.n, t_begin + kSeg) : a.n;
    if (a.mode == 1 && seg + 1 == a.nseg) return;  // (nothing reads the last segment's exit state)
    const unsigned char *in_row = (const unsigned char *)a.in + (u64)row * a.in_stride * (a.in_wide ? 8 : sizeof(T));
    const double *sos = a.sos + row * a.sos_stride, *M = a.M + row * a.m_stride;

    Coef<S> c;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const bool real = (unsigned)i < a.ns;  // behind them: identity sections
        c.b0[i] = real ? sos[6 * i] : 1.0;
        c.b1[i] = real ? sos[6 * i + 1] : 0.0;
        c.b2[i] = real ? sos[6 * i + 2] : 0.0;
        c.a1[i] = real ? sos[6 * i + 4] : 0.0;
        c.a2[i] = real ? sos[6 * i + 5] : 0.0;
    }
    if (tid < (unsigned)D) {
        double e = 0.0;
        if (a.mode == 2) e = a.E[((u64)row * a.nseg + seg) * D + tid];
        else if (a.mode == 0 && a.zi && tid < 2 * a.ns) {
            e = a.zi[row * a.zi_stride + tid];
            if (a.scale) e *= a.scale[row];
        }
        ent[tid] = e;
    }

    for (u64 t0 = t_begin; t0 < t_end; t0 += TILE) {
        const unsigned cnt = (unsigned)min((u64)TILE, t_end - t0), used = (cnt + L - 1) / L;  // work items that own samples
        for (unsigned p = tid; p < TILE; p += 256) {
            const u64 t = t0 + p;
            tile[p + p / L] = p < cnt ? iir_load<T>(a, in_row, BACK ? a.n - 1 - t : t) : 0.0;
        }
        __syncthreads();
        double *mine = tile + tid * LS;
        double z[D];
#pragma unroll
        for (int q = 0; q < D; ++q) z[q] = tid == 0 ? ent[q] : 0.0;
        // pass 1 (work items right of the row's end run on zeros; nothing reads their states)
        for (unsigned i = 0; i < L; ++i) (void)iir_step<S>(c, z, mine[i]);
        // scan: after step j, z = sum over i < 2^(j+1) of M^i exit0(k - i)
        for (unsigned j = 0; j < kLevels && (1u << j) < used; ++j) {
#pragma unroll
            for (int q = 0; q < D; ++q) sc[q * 256 + tid] = z[q];
            __syncthreads();
            if (tid >= (1u << j)) {
                double nb[D];
#pragma unroll
                for (int q = 0; q < D; ++q) nb[q] = sc[q * 256 + tid - (1u << j)];
                iir_link<S>(M + (size_t)j * D * D, nb, z);
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < D; ++q) sc[q * 256 + tid] = z[q];
        __syncthreads();
        if (a.mode != 1) {
            // pass 2, from the exit state of the block to the left
#pragma unroll
            for (int q = 0; q < D; ++q) z[q] = tid == 0 ? ent[q] : sc[q * 256 + tid - 1];
            const unsigned base = tid * L, valid = base < cnt ? min(L, cnt - base) : 0;
            if (valid == L) {
                for (unsigned i = 0; i < L; ++i) mine[i] = iir_step<S>(c, z, mine[i]);
            } else {
                for (unsigned i = 0; i < valid; ++i) mine[i] = iir_step<S>(c, z, mine[i]);
            }
            // the row's state after its last sample
            if (a.zf && t0 + cnt == a.n && tid == used - 1) {
#pragma unroll
                for (int q = 0; q < D; ++q)
                    if ((unsigned)q < 2 * a.ns) a.zf[row * a.zf_stride + q] = z[q];
            }
        }
        __syncthreads();
        if (tid < (unsigned)D) ent[tid] = sc[tid * 256 + 255];  // a whole tile's exit state (a partial tile is the last)
        if (a.mode != 1) {
            unsigned char *out_row = (unsigned char *)a.out + (u64)row * a.out_stride * (a.out_wide ? 8 : sizeof(T));
            for (unsigned p = tid; p < cnt; p += 256) {
                const u64 t = t0 + p, ph = BACK ? a.n - 1 - t : t;
                if (ph < a.out_lo || ph - a.out_lo >= a.out_n) continue;
                const double v = tile[p + p / L];
                if (a.out_wide) ((double *)out_row)[ph - a.out_lo] = v;
                else ((T *)out_row)[ph - a.out_lo] = (T)v;
            }
        }
        __syncthreads();
    }
    if (a.mode == 1 && tid < (unsigned)D) a.E[((u64)row * a.nseg + seg) * D + tid] = ent[tid];
}

// split, launch 2: E[row][s] (segment s's exit state from zero state) -> the segment's entry state, X_s = E_(s-1) + M^(segment) X_(s-1),
// X_0 = the row's entry state; one workgroup of 64 per row, work item r holds component r
__global__ __launch_bounds__(64) void k_iir_link(IirArgs a, unsigned D) {
    __shared__ double x[2 * kMaxS];
    const unsigned row = blockIdx.x, r = threadIdx.x;
    const double *Ms = a.M + row * a.m_stride + (size_t)kLevels * D * D;
    double e = 0.0;
    if (r < D && a.zi && r < 2 * a.ns) {
        e = a.zi[row * a.zi_stride + r];
        if (a.scale) e *= a.scale[row];
    }
    for (unsigned s = 0; s < a.nseg; ++s) {
        double *slot = a.E + ((u64)row * a.nseg + s) * D;
        const double exit0 = r < D ? slot[r] : 0.0;
        if (r < D) { x[r] = e; slot[r] = e; }
        __syncthreads();
        if (r < D) {
            double sum = exit0, err = 0.0;
            for (unsigned q = 0; q < D; ++q) sum = iir_acc2(sum, Ms[r * D + q], x[q], err);
            e = sum + err;
        }
        __syncthreads();
    }
}

// filtfilt: the sample a direction's entry state is scaled by; forward the first extended sample of x, backward the last of the forward pass
template <typename T>
__global__ __launch_bounds__(256) void k_iir_scale(IirArgs a, unsigned rows, unsigned last, double *scale) {
    const unsigned row = blockIdx.x * 256u + threadIdx.x;
    if (row >= rows) return;
    const unsigned char *in_row = (const unsigned char *)a.in + (u64)row * a.in_stride * (a.in_wide ? 8 : sizeof(T));
    scale[row] = iir_load<T>(a, in_row, last ? a.n - 1 : 0);
}

// ---- host tables -----------------------------------------------------------------------------------------------------------------
// one sample through `ns` sections in long double (identity sections behind them leave the sample alone)
inline long double host_step(const double *sos, size_t ns, long double *z, long double x) {
    for (size_t i = 0; i < ns; ++i) {
        const double *s = sos + 6 * i;
        const long double y = (long double)s[0] * x + z[2 * i];
        z[2 * i] = (long double)s[1] * x - (long double)s[4] * y + z[2 * i + 1];
        z[2 * i + 1] = (long double)s[2] * x - (long double)s[5] * y;
        x = y;
    }
    return x;
}

// Pairs of long doubles (value = h + l, |l| <= ulp(h) / 2) for the tables: the recurrence passes through states far larger than the
// entries it ends on when the poles lie close to the circle, and the roundings of 2048 steps in plain long double then show in the last
// bits of an f64 entry.  Error-free sums and products (Knuth, Dekker / Veltkamp with the 2^32 + 1 splitter of a 64-bit significand).
struct DD { long double h, l; };
inline DD dd_norm(long double a, long double b) { const long double s = a + b; return {s, b - (s - a)}; }
inline DD dd_two_sum(long double a, long double b) {
    const long double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
inline DD dd_two_prod(long double a, long double b) {
    const long double C = 4294967297.0L, p = a * b;
    long double t = C * a;
    const long double ah = t - (t - a), al = a - ah;
    t = C * b;
    const long double bh = t - (t - b), bl = b - bh;
    return {p, ((ah * bh - p) + ah * bl + al * bh) + al * bl};
}
inline DD dd_add(DD a, DD b) {
    DD s = dd_two_sum(a.h, b.h);
    s.l += a.l + b.l;
    return dd_norm(s.h, s.l);
}
inline DD dd_mul(double c, DD a) {
    DD p = dd_two_prod((long double)c, a.h);
    p.l += (long double)c * a.l;
    return dd_norm(p.h, p.l);
}
inline void host_step_dd(const double *sos, size_t first, size_t ns, DD *z) {
    DD x{0.0L, 0.0L};
    for (size_t i = first; i < ns; ++i) {  // (the sections in front of the unit state's stay at zero)
        const double *s = sos + 6 * i;
        const DD y = dd_add(dd_mul(s[0], x), z[2 * i]);
        z[2 * i] = dd_add(dd_add(dd_mul(s[1], x), dd_mul(-s[4], y)), z[2 * i + 1]);
        z[2 * i + 1] = dd_add(dd_mul(s[2], x), dd_mul(-s[5], y));
        x = y;
    }
}

// M^(2^j) for j < kLevels (L 2^j samples of zero input, in pairs of long doubles) and, when asked for, M^(segment) (the same run carried on
// in long double): [kLevels + 1][D][D], D = 2 Si, of `ns` real sections
void host_transitions(const double *sos, size_t ns, size_t Si, bool with_segment, double *out) {
    const size_t D = 2 * Si;
    std::fill(out, out + (kLevels + 1) * D * D, 0.0);
    // (the identity sections' states start as zeros and stay zeros: their rows and columns are left as zeros)
    for (size_t col = 0; col < 2 * ns; ++col) {
        DD zd[2 * kMaxS] = {};
        zd[col].h = 1.0L;
        u64 t = 0;
        for (unsigned lvl = 0; lvl < kLevels; ++lvl) {
            for (; t < (u64(kL) << lvl); ++t) host_step_dd(sos, col / 2, ns, zd);
            for (size_t r = 0; r < 2 * ns; ++r) out[(lvl * D + r) * D + col] = (double)(zd[r].h + zd[r].l);
        }
        if (!with_segment) continue;
        long double z[2 * kMaxS];
        for (size_t r = 0; r < 2 * kMaxS; ++r) z[r] = zd[r].h + zd[r].l;
        for (; t < kSeg; ++t) (void)host_step(sos, ns, z, 0.0L);
        for (size_t r = 0; r < 2 * ns; ++r) out[(kLevels * D + r) * D + col] = (double)z[r];
    }
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------------------
struct sgx_iir {
    size_t S = 0, sos_rows = 1, padlen = 0;
    int dtype = SGX_F32, device = -1, route = SGX_IIR_ROUTE_AUTO;
    size_t elem = 4;
    bool chain = false, zi_ok = false;
    std::string zi_err;
    std::vector<double> sos;      // [sos_rows][S][6]
    std::vector<double> zi_unit;  // [sos_rows][S][2]: sosfilt_zi
    struct Pass { size_t first, ns, Si, m_off; };  // sections [first, first + ns) on instance Si; tables at m_off (doubles) of a filter's block
    std::vector<Pass> passes;
    size_t m_row = 0;             // doubles of one filter's tables
    bool with_segment = false;
    std::vector<double> tables;   // [sos_rows][m_row]
    DevBuf d_sos, d_M, d_ziunit, d_state, d_scale, d_E, d_w[2], d_in, d_out, d_zi, d_zf;
    size_t rows = 0;  // rows of the streaming state (0: not fixed)
    size_t allocations = 0;
    const char *last_route = "k_iir_sos";
    mutable std::string err;
};

namespace {

sgx_status grow_counted(sgx_iir *p, DevBuf &b, size_t need) {
    if (b.bytes >= need) return SGX_OK;
    ++p->allocations;
    return grow(p, b, need);
}

size_t instance_for(size_t ns) {
#define SGX_IIR_PICK(S_) if (ns <= S_) return S_;
    SGX_IIR_SECTIONS(SGX_IIR_PICK)
#undef SGX_IIR_PICK
    return 0;
}

size_t lds_bytes(size_t Si) { return (256 * (kL + 1) + 2 * Si * 256) * sizeof(double); }

template <typename T, int S, bool BACK>
hipError_t launch_t(const IirArgs &a, unsigned grid, hipStream_t s) {
    const size_t lds = lds_bytes(S);
    if (lds > 64 * 1024) {
        const hipError_t e = set_max_dynamic_lds((const void *)k_iir_sos<T, S, BACK>, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_iir_sos<T, S, BACK>), dim3(grid), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_sos(int dtype, size_t Si, bool back, const IirArgs &a, unsigned grid, hipStream_t s) {
#define SGX_IIR_LAUNCH(S_)                                                                                           \
    if (Si == S_) {                                                                                                  \
        if (dtype == SGX_F64) return back ? launch_t<double, S_, true>(a, grid, s) : launch_t<double, S_, false>(a, grid, s); \
        return back ? launch_t<float, S_, true>(a, grid, s) : launch_t<float, S_, false>(a, grid, s);                 \
    }
    SGX_IIR_SECTIONS(SGX_IIR_LAUNCH)
#undef SGX_IIR_LAUNCH
    return hipErrorNotSupported;
}

// what one direction of one call runs over
struct Run {
    const void *in; void *out;  // in: used when the direction starts from the caller's rows (cur < 0); out: unless to_work
    size_t in_stride, out_stride;
    bool in_wide, out_wide, back, to_work;  // to_work: the last pass writes a work buffer too (filtfilt's forward direction)
    size_t n, n_in, pad, out_lo, out_n;
    const double *zi; size_t zi_stride;  // [..][S][2], nullptr: zero state
    const double *scale;
    double *zf; size_t zf_stride;
    size_t rows;
};

bool takes_split(const sgx_iir *p, size_t rows, size_t n) {
    if (p->chain) return false;
    if (p->route == SGX_IIR_ROUTE_SPLIT) return true;
    return p->with_segment && rows < kSplitBelowRows && n >= 2 * kSeg;
}
size_t segments_of(size_t n) { return (n + kSeg - 1) / kSeg; }

// scratch of a call: the split route's states, the chain route's and filtfilt's f64 rows
sgx_status scratch_reserve(sgx_iir *p, size_t rows, size_t n, bool filtfilt, size_t pad) {
    sgx_status st;
    const size_t ne = n + (filtfilt ? 2 * pad : 0);
    if (takes_split(p, rows, ne))
        if ((st = grow_counted(p, p->d_E, rows * segments_of(ne) * 2 * kMaxS * sizeof(double))) != SGX_OK) return st;
    const size_t npass = p->passes.size();
    const size_t wide = rows * ne * sizeof(double);
    if (filtfilt || npass > 1)
        if ((st = grow_counted(p, p->d_w[0], wide)) != SGX_OK) return st;
    if (npass > 1 && (filtfilt || npass > 2))
        if ((st = grow_counted(p, p->d_w[1], wide)) != SGX_OK) return st;
    if (filtfilt && (st = grow_counted(p, p->d_scale, rows * sizeof(double))) != SGX_OK) return st;
    return SGX_OK;
}

// one direction: the passes in order.  The first reads r.in (cur < 0) or the work buffer `cur`; every pass but the last writes the
// work buffer its input is not in (f64 rows of r.n samples), the last r.out, or with to_work a work buffer as well; on return `cur`
// names the work buffer written last.
sgx_status run_cascade(sgx_iir *p, const Run &r, int &cur, hipStream_t s) {
    const size_t npass = p->passes.size();
    const bool split = takes_split(p, r.rows, r.n);
    p->last_route = p->chain ? "iir_chain" : split ? "k_iir_sos+split" : "k_iir_sos";
    for (size_t q = 0; q < npass; ++q) {
        const sgx_iir::Pass &ps = p->passes[q];
        IirArgs a{};
        a.n = r.n;
        if (cur < 0) {
            a.in = r.in; a.in_stride = r.in_stride; a.in_wide = r.in_wide; a.pad = unsigned(r.pad); a.n_in = r.n_in;
        } else {
            a.in = p->d_w[cur]; a.in_stride = r.n; a.in_wide = 1; a.n_in = r.n;
        }
        if (q + 1 == npass && !r.to_work) {
            a.out = r.out; a.out_stride = r.out_stride; a.out_wide = r.out_wide; a.out_lo = r.out_lo; a.out_n = r.out_n;
        } else {
            cur = cur == 0 ? 1 : 0;
            a.out = p->d_w[cur]; a.out_stride = r.n; a.out_wide = 1; a.out_lo = 0; a.out_n = r.n;
        }
        a.sos = p->d_sos.as<double>() + ps.first * 6;
        a.sos_stride = p->sos_rows > 1 ? p->S * 6 : 0;
        a.M = p->d_M.as<double>() + ps.m_off;
        a.m_stride = p->sos_rows > 1 ? p->m_row : 0;
        a.zi = r.zi ? r.zi + ps.first * 2 : nullptr;
        a.zi_stride = r.zi_stride;
        a.scale = r.scale;
        a.zf = r.zf ? r.zf + ps.first * 2 : nullptr;
        a.zf_stride = r.zf_stride;
        a.ns = unsigned(ps.ns);
        if (!split) {
            a.mode = 0; a.nseg = 1;
            SGX_TRY_HIP(p, launch_sos(p->dtype, ps.Si, r.back, a, unsigned(r.rows), s));
        } else {
            a.nseg = unsigned(segments_of(r.n));
            a.E = p->d_E.as<double>();
            const unsigned grid = unsigned(r.rows * a.nseg);
            a.mode = 1;
            SGX_TRY_HIP(p, launch_sos(p->dtype, ps.Si, r.back, a, grid, s));
            hipLaunchKernelGGL(k_iir_link, dim3(unsigned(r.rows)), dim3(64), 0, s, a, unsigned(2 * ps.Si));
            SGX_TRY_HIP(p, hipGetLastError());
            a.mode = 2;
            SGX_TRY_HIP(p, launch_sos(p->dtype, ps.Si, r.back, a, grid, s));
        }
    }
    return SGX_OK;
}

sgx_status check_call(sgx_iir *p, const void *x, void *out, size_t batch, size_t n, size_t stride, size_t out_elems, int32_t mem_kind,
                      bool empty_ok) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    if (batch == 0 || (n == 0 && !empty_ok)) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (n && (!x || !out)) return fail(p, SGX_INVALID_INPUT, "Invalid input: null buffer");
    if (stride < n) return fail(p, SGX_INVALID_INPUT, "Invalid input: sample_stride < n_samples");
    if (p->sos_rows > 1 && batch != p->sos_rows) return dim_mismatch(p, p->sos_rows, batch, " (the plan holds one filter per row)");
    if (out_elems != batch * n) return dim_mismatch(p, batch * n, out_elems);
    if (batch > (size_t(1) << 24) || n > (size_t(1) << 40) || batch * segments_of(n + 2 * p->padlen) >= 0x7fffffffull)
        return fail(p, SGX_INVALID_INPUT, "Invalid input: batch or sample count too large");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (mem_kind != SGX_MEM_HOST && mem_kind != SGX_MEM_DEVICE) return fail(p, SGX_INVALID_INPUT, "Invalid input: unknown mem_kind");
    return SGX_OK;
}

// the streaming state for `rows` rows; a new buffer starts as zeros (a call that grows it follows creation or reset)
sgx_status state_reserve(sgx_iir *p, size_t rows, hipStream_t s) {
    const size_t need = rows * p->S * 2 * sizeof(double);
    if (p->d_state.bytes >= need) return SGX_OK;
    const sgx_status st = grow_counted(p, p->d_state, need);
    if (st != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemsetAsync(p->d_state, 0, need, s));
    return SGX_OK;
}

// sgx_iir_filter and sgx_iir_process on device rows
sgx_status filter_dev(sgx_iir *p, const void *x, size_t batch, size_t n, size_t stride, void *out, const double *zi, double *zf, hipStream_t s) {
    sgx_status st = scratch_reserve(p, batch, n, false, 0);
    if (st != SGX_OK) return st;
    Run r{};
    r.in = x; r.out = out; r.in_stride = stride; r.out_stride = n;
    r.n = r.n_in = r.out_n = n;
    r.zi = zi; r.zf = zf; r.zi_stride = r.zf_stride = p->S * 2;
    r.rows = batch;
    int cur = -1;
    return run_cascade(p, r, cur, s);
}

sgx_status filtfilt_dev(sgx_iir *p, const void *x, size_t batch, size_t n, size_t stride, void *out, size_t pad, hipStream_t s) {
    sgx_status st = scratch_reserve(p, batch, n, true, pad);
    if (st != SGX_OK) return st;
    const size_t ne = n + 2 * pad;
    const bool f64 = p->dtype == SGX_F64;
    const unsigned sgrid = unsigned((batch + 255) / 256);
    const size_t zs = p->sos_rows > 1 ? p->S * 2 : 0;
    double *scale = p->d_scale.as<double>();
    // forward over the extended row, from sosfilt_zi * x_ext[0]
    Run r{};
    r.in = x; r.in_stride = stride; r.n = ne; r.n_in = n; r.pad = pad;
    r.to_work = true;
    r.zi = p->d_ziunit.as<double>(); r.zi_stride = zs; r.scale = scale;
    r.rows = batch;
    IirArgs sa{};
    sa.in = x; sa.in_stride = stride; sa.n = ne; sa.n_in = n; sa.pad = unsigned(pad);
    if (f64) hipLaunchKernelGGL(k_iir_scale<double>, dim3(sgrid), dim3(256), 0, s, sa, unsigned(batch), 0u, scale);
    else hipLaunchKernelGGL(k_iir_scale<float>, dim3(sgrid), dim3(256), 0, s, sa, unsigned(batch), 0u, scale);
    SGX_TRY_HIP(p, hipGetLastError());
    int cur = -1;
    if ((st = run_cascade(p, r, cur, s)) != SGX_OK) return st;
    const int fwd = cur;
    // backward over the forward pass, from sosfilt_zi * y[last]; the middle n samples are stored
    Run b{};
    b.in = p->d_w[fwd]; b.in_stride = ne; b.in_wide = true; b.n = b.n_in = ne; b.back = true;
    b.out = out; b.out_stride = n; b.out_lo = pad; b.out_n = n;
    b.zi = p->d_ziunit.as<double>(); b.zi_stride = zs; b.scale = scale;
    b.rows = batch;
    IirArgs sb{};
    sb.in = b.in; sb.in_stride = ne; sb.in_wide = 1; sb.n = sb.n_in = ne;
    hipLaunchKernelGGL(k_iir_scale<double>, dim3(sgrid), dim3(256), 0, s, sb, unsigned(batch), 1u, scale);
    SGX_TRY_HIP(p, hipGetLastError());
    return run_cascade(p, b, cur, s);
}

// scipy.signal.sosfilt_zi of one filter in long double; false with the section's number where (1 + a1 + a2) == 0
bool host_zi(const double *sos, size_t S, double *zi, size_t &bad) {
    long double scale = 1.0L;
    for (size_t i = 0; i < S; ++i) {
        const long double b0 = sos[6 * i], b1 = sos[6 * i + 1], b2 = sos[6 * i + 2], a1 = sos[6 * i + 4], a2 = sos[6 * i + 5];
        const long double det = 1.0L + a1 + a2;
        if (det == 0.0L) { bad = i; return false; }
        const long double B0 = b1 - a1 * b0, B1 = b2 - a2 * b0;
        const long double z0 = (B0 + B1) / det, z1 = B1 - a2 * z0;  // (I - A^T) zi = B, A the companion matrix of a
        zi[2 * i] = double(scale * z0);
        zi[2 * i + 1] = double(scale * z1);
        scale *= (b0 + b1 + b2) / det;
    }
    return true;
}

}  // namespace

extern "C" {

sgx_status sgx_iir_create(const double *sos, size_t n_sections, size_t sos_rows, int32_t route, int32_t dtype, int32_t device,
                          sgx_iir **out) {
    if (out) *out = nullptr;
    auto bad = [&](const std::string &m) { return fail<sgx_iir>(nullptr, SGX_INVALID_INPUT, "Invalid input: " + m); };
    if (!out) return bad("null argument");
    if (n_sections == 0 || !sos) return bad("sos must hold at least one section");
    if (sos_rows == 0) return bad("sos_rows must be > 0");
    if (dtype != SGX_F32 && dtype != SGX_F64) return bad("dtype must be f32 or f64");
    if (route != SGX_IIR_ROUTE_AUTO && route != SGX_IIR_ROUTE_SPLIT && route != SGX_IIR_ROUTE_CHAIN) return bad("unknown route");
    if (n_sections > 4096 || sos_rows > (size_t(1) << 20) || n_sections * sos_rows > (size_t(1) << 22)) return bad("too many sections");
    if (route == SGX_IIR_ROUTE_SPLIT && n_sections > kMaxS) return bad("the split route takes up to 8 sections");
    for (size_t r = 0; r < sos_rows; ++r)
        for (size_t i = 0; i < n_sections; ++i) {
            const double *s = sos + (r * n_sections + i) * 6;
            const std::string where = "section " + std::to_string(i) + (sos_rows > 1 ? " of filter " + std::to_string(r) : "");
            for (int k = 0; k < 6; ++k)
                if (!std::isfinite(s[k])) return bad(where + " has a non-finite coefficient");
            if (s[3] != 1.0) return bad(where + " has a0 = " + std::to_string(s[3]) + " (sections must be normalised to a0 == 1)");
            if (std::fabs(s[5]) > 1.0 || std::fabs(s[4]) > 1.0 + s[5])
                return bad(where + " has a pole outside the unit circle (a1 = " + std::to_string(s[4]) + ", a2 = " + std::to_string(s[5]) + ")");
        }
    sgx_iir *p = new (std::nothrow) sgx_iir();
    if (!p) return fail<sgx_iir>(nullptr, SGX_INTERNAL, "Internal error: out of memory");
    p->S = n_sections; p->sos_rows = sos_rows; p->route = route;
    p->dtype = dtype; p->elem = elem_size(dtype); p->device = device;
    p->chain = route == SGX_IIR_ROUTE_CHAIN || n_sections > kMaxS;
    p->last_route = p->chain ? "iir_chain" : route == SGX_IIR_ROUTE_SPLIT ? "k_iir_sos+split" : "k_iir_sos";
    p->sos.assign(sos, sos + sos_rows * n_sections * 6);
    // scipy's default padlen, the largest over the filters
    for (size_t r = 0; r < sos_rows; ++r) {
        size_t zb = 0, za = 0;
        for (size_t i = 0; i < n_sections; ++i) {
            zb += p->sos[(r * n_sections + i) * 6 + 2] == 0.0;
            za += p->sos[(r * n_sections + i) * 6 + 5] == 0.0;
        }
        p->padlen = std::max(p->padlen, 3 * (2 * n_sections + 1 - std::min(zb, za)));
    }
    p->zi_unit.assign(sos_rows * n_sections * 2, 0.0);
    p->zi_ok = true;
    for (size_t r = 0; r < sos_rows && p->zi_ok; ++r) {
        size_t at = 0;
        if (!host_zi(p->sos.data() + r * n_sections * 6, n_sections, p->zi_unit.data() + r * n_sections * 2, at)) {
            p->zi_ok = false;
            p->zi_err = "Invalid input: sosfilt_zi has no solution: section " + std::to_string(at) + " has a pole at z = 1";
        }
    }
    // passes and their tables
    for (size_t first = 0; first < n_sections; first += kMaxS) {
        const size_t ns = std::min<size_t>(kMaxS, n_sections - first), Si = instance_for(ns);
        p->passes.push_back({first, ns, Si, p->m_row});
        p->m_row += (kLevels + 1) * 4 * Si * Si;
    }
    p->with_segment = !p->chain && (route == SGX_IIR_ROUTE_SPLIT || sos_rows < kSplitBelowRows);
    p->tables.resize(sos_rows * p->m_row);
    for (size_t r = 0; r < sos_rows; ++r)
        for (const auto &ps : p->passes)
            host_transitions(p->sos.data() + (r * n_sections + ps.first) * 6, ps.ns, ps.Si, p->with_segment, p->tables.data() + r * p->m_row + ps.m_off);
    if (device == -2) { *out = p; return SGX_OK; }  // host-only: validation, tables, sosfilt_zi

    auto tables = [&]() -> sgx_status {
        if (device == -1) SGX_TRY_HIP(p, hipGetDevice(&p->device));
        DeviceGuard dg;
        SGX_TRY_HIP(p, dg.enter(p->device));
        sgx_status st;
        if ((st = upload(p, p->d_sos, p->sos, SGX_F64)) != SGX_OK) return st;
        if ((st = upload(p, p->d_M, p->tables, SGX_F64)) != SGX_OK) return st;
        if ((st = upload(p, p->d_ziunit, p->zi_unit, SGX_F64)) != SGX_OK) return st;
        return SGX_OK;
    };
    return finish_create(p, tables(), out, sgx_iir_destroy);
}

void sgx_iir_destroy(sgx_iir *p) {
    if (!p) return;
    DeviceGuard dg;
    if (p->device != -2) (void)dg.enter(p->device);
    delete p;
}

sgx_status sgx_iir_filter(sgx_iir *p, const void *x, size_t batch, size_t n, size_t stride, void *out, size_t out_elems, const double *zi,
                          double *zf, int32_t mem_kind, void *stream) {
    sgx_status st = check_call(p, x, out, batch, n, stride, out_elems, mem_kind, false);
    if (st != SGX_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return filter_dev(p, x, batch, n, stride, out, zi, zf, s);
    const size_t in_bytes = ((batch - 1) * stride + n) * p->elem, out_bytes = out_elems * p->elem, z_bytes = batch * p->S * 2 * sizeof(double);
    if ((st = grow_counted(p, p->d_in, in_bytes)) != SGX_OK || (st = grow_counted(p, p->d_out, out_bytes)) != SGX_OK) return st;
    if ((st = grow_counted(p, p->d_zi, z_bytes)) != SGX_OK || (st = grow_counted(p, p->d_zf, z_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
    if (zi) SGX_TRY_HIP(p, hipMemcpyAsync(p->d_zi, zi, z_bytes, hipMemcpyHostToDevice, s));
    if ((st = filter_dev(p, p->d_in, batch, n, stride, p->d_out, zi ? p->d_zi.as<double>() : nullptr, zf ? p->d_zf.as<double>() : nullptr, s)) != SGX_OK)
        return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    if (zf) SGX_TRY_HIP(p, hipMemcpyAsync(zf, p->d_zf, z_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

sgx_status sgx_iir_process(sgx_iir *p, const void *x, size_t batch, size_t n, size_t stride, void *out, size_t out_elems, int32_t mem_kind,
                           void *stream) {
    sgx_status st = check_call(p, x, out, batch, n, stride, out_elems, mem_kind, true);
    if (st != SGX_OK) return st;
    if (p->rows && batch != p->rows) return dim_mismatch(p, p->rows, batch, " (rows of the state; reset() releases them)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if ((st = state_reserve(p, batch, s)) != SGX_OK) return st;
    p->rows = batch;
    if (n == 0) return SGX_OK;
    double *z = p->d_state.as<double>();
    if (mem_kind == SGX_MEM_DEVICE) return filter_dev(p, x, batch, n, stride, out, z, z, s);
    const size_t in_bytes = ((batch - 1) * stride + n) * p->elem, out_bytes = out_elems * p->elem;
    if ((st = grow_counted(p, p->d_in, in_bytes)) != SGX_OK || (st = grow_counted(p, p->d_out, out_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
    if ((st = filter_dev(p, p->d_in, batch, n, stride, p->d_out, z, z, s)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

sgx_status sgx_iir_filtfilt(sgx_iir *p, const void *x, size_t batch, size_t n, size_t stride, void *out, size_t out_elems, int64_t padlen,
                            int32_t mem_kind, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    const size_t pad = padlen < 0 ? p->padlen : size_t(padlen);
    if (n <= pad)
        return fail(p, SGX_INVALID_INPUT, "Invalid input: the length of the input (" + std::to_string(n) + ") must be greater than padlen (" +
                                              std::to_string(pad) + ")");
    if (pad > (size_t(1) << 30)) return fail(p, SGX_INVALID_INPUT, "Invalid input: padlen too large");
    if (!p->zi_ok) return fail(p, SGX_INVALID_INPUT, p->zi_err);
    sgx_status st = check_call(p, x, out, batch, n, stride, out_elems, mem_kind, false);
    if (st != SGX_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    if (mem_kind == SGX_MEM_DEVICE) return filtfilt_dev(p, x, batch, n, stride, out, pad, s);
    const size_t in_bytes = ((batch - 1) * stride + n) * p->elem, out_bytes = out_elems * p->elem;
    if ((st = grow_counted(p, p->d_in, in_bytes)) != SGX_OK || (st = grow_counted(p, p->d_out, out_bytes)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_in, x, in_bytes, hipMemcpyHostToDevice, s));
    if ((st = filtfilt_dev(p, p->d_in, batch, n, stride, p->d_out, pad, s)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(out, p->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

sgx_status sgx_iir_reset(sgx_iir *p, void *stream) {
    if (!p) return fail(p, SGX_INVALID_INPUT, "Invalid input: null plan");
    p->rows = 0;
    if (p->device == -2 || !p->d_state.ptr) return SGX_OK;
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    SGX_TRY_HIP(p, hipMemsetAsync(p->d_state, 0, p->d_state.bytes, static_cast<hipStream_t>(stream)));
    return SGX_OK;
}

sgx_status sgx_iir_state(sgx_iir *p, double *z, size_t z_elems, void *stream) {
    if (!p || !z) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (p->rows == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: the plan holds no state (no process() or set_state() since reset)");
    if (z_elems != p->rows * p->S * 2) return dim_mismatch(p, p->rows * p->S * 2, z_elems);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    SGX_TRY_HIP(p, hipMemcpyAsync(z, p->d_state, z_elems * sizeof(double), hipMemcpyDeviceToHost, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    return SGX_OK;
}

sgx_status sgx_iir_set_state(sgx_iir *p, const double *z, size_t rows, void *stream) {
    if (!p || !z || rows == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument or no rows");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (p->sos_rows > 1 && rows != p->sos_rows) return dim_mismatch(p, p->sos_rows, rows, " (the plan holds one filter per row)");
    if (p->rows && rows != p->rows) return dim_mismatch(p, p->rows, rows, " (rows of the state; reset() releases them)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st = state_reserve(p, rows, s);
    if (st != SGX_OK) return st;
    SGX_TRY_HIP(p, hipMemcpyAsync(p->d_state, z, rows * p->S * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    SGX_TRY_HIP(p, hipStreamSynchronize(s));
    p->rows = rows;
    return SGX_OK;
}

sgx_status sgx_iir_reserve(sgx_iir *p, size_t batch, size_t n, int32_t host_staging) {
    if (!p || batch == 0 || n == 0) return fail(p, SGX_INVALID_INPUT, "Invalid input: samples must be non-empty");
    if (p->device == -2) return fail(p, SGX_BACKEND, kNoDeviceText);
    if (p->rows && batch > p->rows) return dim_mismatch(p, p->rows, batch, " (rows of the state; reset() releases them)");
    DeviceGuard dg;
    SGX_TRY_HIP(p, dg.enter(p->device));
    sgx_status st;
    if ((st = state_reserve(p, batch, nullptr)) != SGX_OK) return st;
    SGX_TRY_HIP(p, hipStreamSynchronize(nullptr));
    if ((st = scratch_reserve(p, batch, n, false, 0)) != SGX_OK) return st;
    if (p->zi_ok && (st = scratch_reserve(p, batch, n, true, p->padlen)) != SGX_OK) return st;
    if (host_staging) {
        const size_t z_bytes = batch * p->S * 2 * sizeof(double);
        if ((st = grow_counted(p, p->d_in, batch * n * p->elem)) != SGX_OK || (st = grow_counted(p, p->d_out, batch * n * p->elem)) != SGX_OK) return st;
        if ((st = grow_counted(p, p->d_zi, z_bytes)) != SGX_OK || (st = grow_counted(p, p->d_zf, z_bytes)) != SGX_OK) return st;
    }
    return SGX_OK;
}

sgx_status sgx_iir_transition(const sgx_iir *p, int32_t j, double *m) {
    if (!p || !m) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (j < 0 || j >= int32_t(kLevels)) return fail(p, SGX_INVALID_INPUT, "Invalid input: j must be 0 .. 7");
    const sgx_iir::Pass &ps = p->passes[0];
    const size_t D = 2 * ps.Si, d = 2 * ps.ns;
    const double *t = p->tables.data() + ps.m_off + size_t(j) * D * D;
    for (size_t r = 0; r < d; ++r)
        for (size_t q = 0; q < d; ++q) m[r * d + q] = t[r * D + q];
    return SGX_OK;
}

sgx_status sgx_iir_zi(const sgx_iir *p, double *zi) {
    if (!p || !zi) return fail(p, SGX_INVALID_INPUT, "Invalid input: null argument");
    if (!p->zi_ok) return fail(p, SGX_INVALID_INPUT, p->zi_err);
    std::copy(p->zi_unit.begin(), p->zi_unit.end(), zi);
    return SGX_OK;
}

size_t sgx_iir_n_sections(const sgx_iir *p) { return p ? p->S : 0; }
size_t sgx_iir_padlen(const sgx_iir *p) { return p ? p->padlen : 0; }
size_t sgx_iir_tile(const sgx_iir *p) { return p && !p->chain ? kTile : 0; }
size_t sgx_iir_block(const sgx_iir *p) { return p ? kL : 0; }
size_t sgx_iir_allocations(const sgx_iir *p) { return p ? p->allocations : 0; }
const char *sgx_iir_kernel_name(const sgx_iir *p) { return p ? p->last_route : ""; }
int32_t sgx_iir_device(const sgx_iir *p) { return p ? p->device : -2; }
const char *sgx_iir_last_error(const sgx_iir *p) { return p ? p->err.c_str() : create_err<sgx_iir>().c_str(); }

}  // extern "C"

// plan_host.h — the host-side scaffold every plan family of libspectro_hip.so shares: error storage, the HIP error macro, owning
// device buffers with their growth and table upload, the inner-plan handle and the create epilogue.  Host code only.
#pragma once

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "sgx_internal.h"

namespace sgx {

// Device memory a plan owns.  It reads as its pointer where a void * argument is expected (so a HIP call's text in an error message
// names the buffer as before); a test for "allocated" names `.ptr`.  The destructor frees it, so the plan is deleted with its device
// current (DeviceGuard).
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (ptr) (void)hipFree(ptr);
    }
    operator void *() const { return ptr; }
    explicit operator bool() const = delete;
    template <typename T>
    T *as() const { return static_cast<T *>(ptr); }
};

}  // namespace sgx

struct sgx_plan {
    sgx_params p{};
    std::vector<double> custom_window;
    int device = -1;       // -2: host-only plan
    bool device_ready = false;
    int dtype = SGX_F32;
    size_t elem = 4;
    unsigned nb_fft = 0, n_out = 0;
    int out_mode = 0, amp = 0;
    double eps = 0.0;
    sgx::KernelKind kind = sgx::K_DIRECT_DFT;

    // host tables (f64, as the reference builds them)
    std::vector<double> window;
    std::vector<uint32_t> mel_ptr, mel_col;
    std::vector<double> mel_val;
    std::vector<double> loghz_freqs;  // LogHz / ERB axis (centre frequencies), empty otherwise

    // device tables
    void *d_window = nullptr, *d_tw = nullptr, *d_tw1 = nullptr, *d_tw2 = nullptr;
    void *d_mel_ptr = nullptr, *d_mel_col = nullptr, *d_mel_val = nullptr, *d_mel_pptr = nullptr, *d_mel_pcol = nullptr, *d_mel_pw = nullptr, *d_mm_frag = nullptr, *d_mm_blk = nullptr, *d_mel_sched = nullptr;
    unsigned mel_sched_words = 0;
    std::vector<uint32_t> h_mel_sched;  // the tuned kernel's band schedule as built on the host (plan.hip build_band_schedule)
    unsigned mm_nblk = 0;
    unsigned mel_pchunks = 0;
    unsigned mel_contig = 0;
    void *d_ones = nullptr;  // rectangular window for sgx_r2c
    // MFCC epilogue: DCT-II basis [n_mfcc][n_mels] and lifter [n_mfcc] in T; Mel-dB scratch (grown on demand)
    void *d_dct = nullptr, *d_lifter = nullptr;
    sgx::DevBuf d_melbuf;
    void *d_mfcc_frag = nullptr;  // fused MFCC epilogue of the tuned f32 kernel: the basis as matrix-core fragments (null: separate launch)
    unsigned mfcc_frag_words = 0, mfcc_steps = 0, mfcc_mtiles = 0;
    // split filterbank path (long frames): the per-bin power / magnitude tensor between the two launches (grown on demand)
    sgx::DevBuf d_pwbuf;
    bool split_bank = false;  // decided at plan creation (plan.hip)
    unsigned n_final = 0;  // rows of the final output (n_out, or the MFCC row count)
    void *d_window_half = nullptr, *d_ones_half = nullptr;  // 0.5*window (exact) for the tuned kernel's real split
    // inverse path (sgx_istft / sgx_c2r), created on first use: full twiddle table e^{-2 pi i k/n}, frame scratch, flag
    void *d_itw = nullptr, *d_flag = nullptr;
    sgx::DevBuf d_frames;
    void *d_itwr = nullptr, *d_itw1 = nullptr;  // tables of the plan's fused inverse of a single shape, if it has one (plan.hip kFusedInverse)
    // K_BLUESTEIN: chirp, transformed chirp, length-M twiddles (the sequences themselves never leave LDS: no frame scratch)
    void *d_bs_chirp = nullptr, *d_bs_tw = nullptr, *d_bs_wc = nullptr, *d_bs_bhp = nullptr;
    unsigned bs_M = 0;
    bool bs_fwd_half = false;  // K_BLUESTEIN in half-length complex form (even n_fft whose own convolution does not fit LDS)
    sgx::BsDevTables bs_half;  // inverse rows of an even n_fft whose own chirp-z does not fit: tables of length n_fft / 2 (inverse_tables)
    const char *bank_stage = "", *bank_epilogue = "";  // filterbank stage (+ MFCC launch) of the last successful execute (sgx_bank_stage_name): "" before any / without a bank
    mutable std::string bank_stage_text;               // the two put together for the caller
    const char *istft_route = "";  // route of the last successful sgx_istft / sgx_c2r (sgx_istft_kernel_name): "" before any
    const char *exec_route = "";   // kernel of the last successful forward launch, after the chain (sgx_execute_kernel_name): "" before any
    // K_BIGFFT: tables of the global-memory transforms and their sequence scratch (grown on demand, pre-sized by sgx_reserve)
    sgx::BigDev big;
    unsigned big_n = 0;  // set at creation when the plan's kind is K_BIGFFT (host-only plans have no tables)
    sgx::DevBuf d_big;

    // K_CQT: kernels as built (f64, packed bin after bin), centre frequencies, the device layout (cqt.hip) and its LDS tiling
    std::vector<uint32_t> cqt_len;
    std::vector<double> cqt_re, cqt_im, cqt_freqs;
    unsigned cqt_groups = 0, cqt_lpad = 0, cqt_m = 0;
    void *d_cqt_tab = nullptr, *d_cqt_info = nullptr, *d_cqt_len = nullptr;
    // transform plans (sgx_plan_create_cqt_transform): cqt()'s framing and bin rule; one-frame calls take the rows route unless
    // sgx_cqt_set_route asked for the per-signal tiles; sgx_kernel_name reports the route of the last call
    bool cqt_transform = false, cqt_rows_last = false;
    int cqt_route = 0;

    // plan-owned staging for host-pointer execution
    sgx::DevBuf d_in, d_out;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    mutable std::string err;
    mutable size_t dm_expected = 0, dm_got = 0;  // the last DimensionMismatch{expected, got} (src/error.rs:19-21)
};

namespace sgx {

constexpr const char *kNoDeviceText = "hip -- FFT backend error: plan has no HIP device (host-only plan)";

inline size_t elem_size(int dtype) { return dtype == SGX_F64 ? 8 : 4; }

// Workgroups of a grid-stride kernel over `total` items: 256 threads each, at most 2^20 of them (the kernels walk the rest).
// (stream.hip / istream.hip cap theirs at 2048 workgroups: a different rule, kept there as grid_for.)
inline unsigned grid_for_items(unsigned long long total) {
    const unsigned long long g = (total + 255) / 256, cap = 1ull << 20;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// The per-thread text of plan type P's last failed create; <prefix>_last_error(NULL) reads it.
template <typename P>
std::string &create_err() {
    thread_local std::string text;
    return text;
}

// An error goes to the plan, or without one to the type's create-error text.
template <typename P>
sgx_status fail(const P *p, sgx_status st, const std::string &msg) {
    if (p) p->err = msg; else create_err<P>() = msg;
    return st;
}
// sgx_plan: a call without a plan leaves sgx_last_create_error() alone; only a failed create writes it (plan.hip create_fail, open_plan)
template <>
inline sgx_status fail<sgx_plan>(const sgx_plan *p, sgx_status st, const std::string &msg) {
    if (p) p->err = msg;
    return st;
}

#define SGX_TRY_HIP(plan, call)                                                                                                  \
    do {                                                                                                                         \
        hipError_t e_ = (call);                                                                                                  \
        if (e_ != hipSuccess)                                                                                                    \
            return sgx::fail(plan, SGX_BACKEND, std::string("hip -- FFT backend error: ") + #call + ": " + hipGetErrorString(e_)); \
    } while (0)

// DimensionMismatch{expected, got} (src/error.rs:19-21); `note` follows the numbers where a site explains them.  An sgx_plan also
// keeps the two numbers (sgx_last_dim_mismatch).
template <typename P>
sgx_status dim_mismatch(const P *p, size_t expected, size_t got, const std::string &note = "") {
    if constexpr (std::is_same_v<P, sgx_plan>) {
        if (p) { p->dm_expected = expected; p->dm_got = got; }
    }
    return fail(p, SGX_DIM_MISMATCH, "Dimension mismatch: expected " + std::to_string(expected) + ", got " + std::to_string(got) + note);
}

// scratch of at least `need` bytes; a buffer that is large enough is left alone (a reserved call allocates nothing)
template <typename P>
sgx_status grow(P *p, DevBuf &b, size_t need) {
    if (b.bytes >= need) return SGX_OK;
    if (b.ptr) SGX_TRY_HIP(p, hipFree(b.ptr));
    b.ptr = nullptr;
    b.bytes = 0;
    SGX_TRY_HIP(p, hipMalloc(&b.ptr, need));
    b.bytes = need;
    return SGX_OK;
}

// a host table built in f64, on the device in the type of `dtype` (T::from_f64); an empty table stays a null pointer
template <typename P>
sgx_status upload(P *p, void **dst, const std::vector<double> &src, int dtype) {
    *dst = nullptr;
    if (src.empty()) return SGX_OK;
    const size_t bytes = src.size() * elem_size(dtype);
    std::vector<float> f32;
    if (dtype != SGX_F64) f32.assign(src.begin(), src.end());
    SGX_TRY_HIP(p, hipMalloc(dst, bytes));
    SGX_TRY_HIP(p, hipMemcpy(*dst, dtype == SGX_F64 ? (const void *)src.data() : (const void *)f32.data(), bytes, hipMemcpyHostToDevice));
    return SGX_OK;
}
template <typename P>
sgx_status upload(P *p, DevBuf &b, const std::vector<double> &src, int dtype) {
    const sgx_status st = upload(p, &b.ptr, src, dtype);
    if (st == SGX_OK) b.bytes = src.size() * elem_size(dtype);
    return st;
}

// chirp-z tables of bluestein_host_tables; the launchers read the raw pointers, the owning plan's destroy calls bs_free
template <typename P>
sgx_status upload_bs(P *p, BsDevTables &d, const BsHostTables &h, int dtype) {
    sgx_status st;
    if ((st = upload(p, &d.chirp, h.chirp, dtype)) != SGX_OK) return st;
    if ((st = upload(p, &d.bhp, h.bhp, dtype)) != SGX_OK) return st;
    if ((st = upload(p, &d.tw, h.tw, dtype)) != SGX_OK) return st;
    d.M = h.M;
    return SGX_OK;
}
inline void bs_free(BsDevTables &d) {
    for (void **t : {&d.chirp, &d.bhp, &d.tw}) {
        if (*t) (void)hipFree(*t);
        *t = nullptr;
    }
    d.M = 0;
}

// a plan that owns another sgx_plan
struct PlanDeleter {
    void operator()(sgx_plan *p) const { sgx_plan_destroy(p); }
};
using PlanHandle = std::unique_ptr<sgx_plan, PlanDeleter>;

// One frame of n samples per row: sgx_execute is a batched R2C, sgx_istft a batched C2R (n_fft = hop = n, rectangular window, not
// centred, complex output).  A failure leaves its text in sgx_last_create_error().
inline sgx_status create_row_fft(size_t n, int dtype, int device, PlanHandle &plan) {
    sgx_params sp{};
    sp.n_fft = uint32_t(n); sp.hop_size = uint32_t(n); sp.centre = 0;
    sp.window_kind = SGX_WIN_RECTANGULAR;
    sp.sample_rate_hz = 1.0;
    sp.freq_scale = SGX_FREQ_LINEAR; sp.amp_scale = SGX_AMP_COMPLEX;
    sp.dtype = dtype; sp.device = device;
    sgx_plan *raw = nullptr;
    const sgx_status st = sgx_plan_create(&sp, &raw);
    plan.reset(raw);
    return st;
}

// The end of a create function: hand the plan out, or keep its error text as the type's create error and destroy it.
template <typename P, typename Destroy>
sgx_status finish_create(P *p, sgx_status st, P **out, Destroy destroy) {
    if (st != SGX_OK) {
        create_err<P>() = p->err;
        destroy(p);
        return st;
    }
    *out = p;
    return SGX_OK;
}

}  // namespace sgx

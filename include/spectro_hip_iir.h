/* spectro_hip_iir.h — batched IIR filtering plans (sgx_iir_*) of libspectro_hip.so: cascades of second-order sections along whole
 * rows, after scipy.signal.sosfilt / sosfiltfilt, for real rows in f32 and f64.
 *
 * This header stands beside spectro_hip.h (which does not include it) and takes from it sgx_status, the SGX_F32 / SGX_F64 and
 * SGX_MEM_* constants, the general rules (no abort across the ABI, no CPU fallback, no global state) and the stream contract: every
 * call below that takes a `stream` enqueues all of its work on that stream and on nothing else and returns without waiting for it;
 * a device-pointer call that fits what sgx_iir_reserve sized allocates nothing, does not synchronise, copies nothing from the host
 * and can be captured into a hipGraph and replayed; a call that has to grow scratch frees and allocates.  A call does not depend on
 * the calls before it, except for the state sgx_iir_process exists to carry.  A plan is used by one caller at a time.
 *
 * Filter.  sos[S][6] = (b0, b1, b2, a0, a1, a2) per section with a0 == 1, S >= 1; one filter for every row (sos_rows = 1) or
 * sos[rows][S][6], one per row of every call.  Each section runs in Direct Form II transposed in f64 for both dtypes, each product
 * and sum rounded on its own (no fused multiply-add), the sections in order:
 *     y = b0 x + z0;   z0 = b1 x - a1 y + z1;   z1 = b2 x - a2 y
 * Samples are widened to f64 going in and rounded to the plan's type once coming out.  The state z[rows][S][2] (f64) has the meaning
 * and the layout of scipy's zi / zf per row.  Create rejects S = 0, a non-finite coefficient, a0 != 1 and a section with a pole
 * strictly outside the unit circle (|a2| > 1 or |a1| > 1 + a2; poles on the circle pass), naming the section.
 *
 * Algorithm.  A workgroup of 256 work items takes a tile of sgx_iir_tile = 256 L consecutive samples of one row, L = sgx_iir_block
 * per work item: every work item runs the cascade over its block from zero state (the first from the tile's entry state), the 256
 * exit states are linked by a log-step scan s_k += M^(2^j) s_(k - 2^j) with the block's 2S x 2S state-transition tables (evaluated
 * at plan time by running the recurrence itself in pairs of long doubles, sgx_iir_transition; the scan's dot products are carried in
 * twice the working precision and rounded once), and every work item runs its block again from its true entry state.  The result
 * is the sequential recurrence's up to the rounding of the linked states; it is not bit-equal to it, and because the block boundaries lie where a call's samples begin, sgx_iir_process over pushes agrees with one sgx_iir_filter
 * call over the concatenation to within that rounding and not bit for bit: THE BLOCK BOUNDARIES MOVE WITH THE PUSHES.  The first
 * min(n, L) samples of a call are the sequential recurrence's bit for bit.
 *
 * Routes (sgx_iir_kernel_name, of the last call; before any call the route an "auto" plan starts with):
 *   "k_iir_sos"        one launch; a workgroup walks the tiles of its row in order, the state stays on chip.
 *   "k_iir_sos+split"  few long rows: a row is cut into segments of SGX_IIR_SEGMENT_TILES tiles; launch 1 computes every segment's
 *                      exit state from zero state, launch 2 chains them per row through the plan-time table M^(segment), launch 3
 *                      filters every segment from its true entry state.  "auto" takes it for fewer than 128 rows of at least two
 *                      segments.
 *   "iir_chain"        S above 8 (or when asked for): consecutive passes of at most 8 sections through f64 scratch; the
 *                      arithmetic is that of one cascade.
 * No workgroup waits on another inside a launch.  Within a route a row's bits depend on neither the batch size nor the other rows.
 *
 * Non-finite samples: everything before a row's first non-finite sample is unaffected and other rows are unaffected bit for bit;
 * from that sample on a recursive filter's row is NaN, as the recurrence itself gives; where the recurrence would recover (a section
 * without feedback) the rest of the row may still be NaN.
 *
 * sgx_iir_filtfilt is scipy.signal.sosfiltfilt with padtype = "odd": the row is extended by padlen samples on both sides
 * (2 x[0] - x[padlen - i] and 2 x[n - 1] - x[n - 2 - m], formed in f64 as the samples are loaded: no extended copy exists), filtered
 * forward from sosfilt_zi * x_ext[0] into f64 scratch, filtered backward from sosfilt_zi * y[last] (the kernel walks the row from its
 * end: no flipped copy exists) and trimmed.  padlen < 0 asks for the default, sgx_iir_padlen =
 * 3 (2 S + 1 - min(#sections with b2 == 0, #sections with a2 == 0)) (for one filter per row: the largest over the rows);
 * n_samples <= padlen is SGX_INVALID_INPUT, as is a filter for which sosfilt_zi has no solution (a pole at z = 1).
 */
#ifndef SPECTRO_HIP_IIR_H
#define SPECTRO_HIP_IIR_H

#include "spectro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SGX_IIR_ROUTE_AUTO = 0, SGX_IIR_ROUTE_SPLIT = 1, SGX_IIR_ROUTE_CHAIN = 2 };
#define SGX_IIR_SEGMENT_TILES 8

typedef struct sgx_iir sgx_iir; /* opaque */

/* device: a HIP ordinal, -1 the current device, -2 a host-only plan (validation, tables, sosfilt_zi; compute calls return SGX_BACKEND) */
sgx_status sgx_iir_create(const double *sos, size_t n_sections, size_t sos_rows, int32_t route, int32_t dtype, int32_t device,
                          sgx_iir **out);
void sgx_iir_destroy(sgx_iir *plan);

/* stateless: x [batch][n_samples] (rows sample_stride apart) -> out [batch][n_samples], from zero state or from zi [batch][S][2];
 * zf [batch][S][2] receives the final state; zi and zf may be NULL, are f64 and live where mem_kind says x and out do */
sgx_status sgx_iir_filter(sgx_iir *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                          size_t out_elems, const double *zi, double *zf, int32_t mem_kind, void *stream);
/* streaming: as sgx_iir_filter from the plan's per-row state, which it replaces in stream order; n_samples may be 0.  The first call
 * after creation or sgx_iir_reset fixes the row count. */
sgx_status sgx_iir_process(sgx_iir *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                           size_t out_elems, int32_t mem_kind, void *stream);
sgx_status sgx_iir_filtfilt(sgx_iir *plan, const void *x, size_t batch, size_t n_samples, size_t sample_stride, void *out,
                            size_t out_elems, int64_t padlen, int32_t mem_kind, void *stream);
/* zero state, and the row count of the next sgx_iir_process is free again */
sgx_status sgx_iir_reset(sgx_iir *plan, void *stream);
/* the streaming state [rows][S][2] to and from host memory, behind what is queued on `stream` (these two wait for it);
 * sgx_iir_set_state fixes the row count as a first sgx_iir_process does */
sgx_status sgx_iir_state(sgx_iir *plan, double *z, size_t z_elems, void *stream);
sgx_status sgx_iir_set_state(sgx_iir *plan, const double *z, size_t rows, void *stream);
/* pre-size state and scratch for calls of up to `batch` rows of `n_samples` samples on every entry point above */
sgx_status sgx_iir_reserve(sgx_iir *plan, size_t batch, size_t n_samples, int32_t host_staging);

/* M^(2^j), j = 0 .. 7, of the first filter's first min(S, 8) sections over one block of L samples: m [2 S'][2 S'] row-major,
 * state_after = m state_before with zero input */
sgx_status sgx_iir_transition(const sgx_iir *plan, int32_t j, double *m);
/* scipy.signal.sosfilt_zi of every filter: zi [sos_rows][S][2], solved in long double */
sgx_status sgx_iir_zi(const sgx_iir *plan, double *zi);

size_t sgx_iir_n_sections(const sgx_iir *plan);
size_t sgx_iir_padlen(const sgx_iir *plan);
size_t sgx_iir_tile(const sgx_iir *plan);  /* 256 L; 0 on the chain route */
size_t sgx_iir_block(const sgx_iir *plan); /* L */
size_t sgx_iir_allocations(const sgx_iir *plan); /* (re)allocations of plan-owned device buffers since creation */
const char *sgx_iir_kernel_name(const sgx_iir *plan);
int32_t sgx_iir_device(const sgx_iir *plan);
const char *sgx_iir_last_error(const sgx_iir *plan); /* NULL plan: the text of the last failed create */

#ifdef __cplusplus
}
#endif

#endif /* SPECTRO_HIP_IIR_H */

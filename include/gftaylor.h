/* gftaylor — C ABI of the MI355X-native multivariate-Taylor arithmetic core.
 *
 * This is the drop-in boundary for the hot path of fzaiser/genfer: the `TaylorPoly<T>` type of
 * src/multivariate_taylor.rs, instantiated at T = F64 (prefix gft_) and T = Interval<F64>
 * (prefix gfti_, `--bounds`).  The reference has no FFI today (the boundary is a Rust generic
 * used only by src/generating_function.rs:8); each entry point below replaces one Rust item and
 * cites it as `mt:<lines>` (= src/multivariate_taylor.rs).  INTEGRATION.md shows the Rust
 * `extern "C"` block + newtype shim a maintainer would add.
 *
 * Model
 *   - A polynomial is an opaque handle (`gft_poly*`).  Its coefficient tensor lives in HBM as a
 *     contiguous row-major f64 array of the *compact* stored shape (mt:13-19); `degrees_p1`
 *     (conceptual truncation orders, SIZE_MAX = untruncated) lives on the host.
 *   - Value arithmetic runs in HIP kernels on gfx950.  There is no CPU fallback: if no device /
 *     code object is available every call fails and gft_last_error() says why.
 *   - Size-threshold dispatch: Genfer issues 10^5-10^6 operations on tensors of a
 *     few hundred elements, each far below a kernel launch.  A tensor with at most
 *     "host_max_elems" elements whose operands are all host-resident (built from host data or by
 *     such operations) stays in host memory and is computed there by the same element functions
 *     the kernels use (one source, same bits, -ffp-contract=off); scalars never leave the host.
 *     A host-resident tensor that meets a device operand is mirrored to the device once.
 *     gft_set_option("host_max_elems", 0) keeps every tensor on the device.
 *   - The ABI is NON-consuming: `out = op(a, b)` never frees or mutates its inputs (the Rust
 *     operators consume by value, mt:857,914,1017,1197; a shim maps that to "call, then drop").
 *     Handles are immutable values; gft_clone is O(1) (shared device buffer).
 *   - Kernel launches are issued by a LAUNCH THREAD of the library, in program order (a launch-bound program spends ~3 us
 *     of host time inside every hipLaunchKernel; the calling thread only records the launch).  Every value inspection,
 *     gft_synchronize, gft_event_record and the raw entry points gft_conv_raw* / gft_dist_* return with all launches in
 *     the stream; a caller that shares the stream with the HANDLE API (gft_set_stream) and records its own events or
 *     launches its own kernels there calls gft_synchronize() or gft_event_record() first.
 *   - Single calling thread per process; one HIP stream (gft_set_stream to adopt the caller's).
 *     The host only synchronises when a VALUE is inspected (to_host, coefficient, constant_term,
 *     is_zero/is_one/extract_*, equal) — and data-dependent dispatch inside mul/div/subst_var
 *     (mt:1021-1061), which the reference also performs.
 *   - Stored (compact) shapes and degrees_p1 equal the reference's in every case (integer
 *     bookkeeping is bit-exact); subst_var's Horner loop speculates on the data-dependent dispatch
 *     of mt:1052-1061 on the device, verifies the speculation with one read-back per call and
 *     redoes the loop step by step if it failed.
 *   - Errors: functions returning a handle return NULL, functions returning int return a
 *     negative value; gft_last_error() holds the message.  Reference panics (assert!/unwrap,
 *     `panic = "abort"`, Cargo.toml:29) map to such errors; IEEE inf/NaN propagate as values.
 *   - Scalars cross the boundary as `const double*` pointing at WIDTH doubles: 1 for gft_
 *     (the f64), 2 for gfti_ ({lo, hi}).  Coefficient data is plane-major: WIDTH planes of
 *     numel doubles each (SoA (lo,hi) planes for intervals).
 */
#ifndef GFTAYLOR_H
#define GFTAYLOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gft_poly gft_poly;

/* ---- runtime ------------------------------------------------------------------------- */
/* Select the HIP device and create the stream + memory pool.  Idempotent. 0 on success. */
int gft_init(int device);
void gft_shutdown(void);
/* Adopt an existing hipStream_t (e.g. torch's current stream); NULL restores the library's own. */
int gft_set_stream(void* hip_stream);
void* gft_get_stream(void);
/* The HIP device ordinal the library runs on (gft_init(-1) first if nothing has initialised it); -1 on failure. */
int gft_device(void);
int gft_synchronize(void);
const char* gft_last_error(void);
/* Device-memory statistics in bytes: {in_use, cached, peak_in_use}.  in_use and peak include the kernels' grow-only
 * workspaces (the row-pair sums of the reference-order product, at most conv_rb_pairs_cap = 2 GiB over all streams; the tiled
 * product's plan workspace), which are not pool blocks. */
void gft_pool_stats(size_t out[3]);
/* Cumulative operation counters since gft_init: {extract_linear device scans (each a host round trip),
 * 1-element value read-backs, coefficient() read-backs, products on the tiled kernel, on the LDS-staged
 * reference-order kernel, on the one-thread-per-output kernel, operations computed on the host tier,
 * host-resident tensors mirrored to the device}.  Diagnostics. */
void gft_op_stats(size_t out[8]);
/* More counters (returns how many exist — 18 — and writes min(cap, that many)): {kernel launches of the library, elementwise
 * operations deferred into a chain instead of launched, chains materialised by a consumer that needed the tensor in
 * memory, add/sub launches that evaluated deferred chains on the fly, launches whose argument block did not fit a
 * slot of the launch ring and were issued in place after a full drain, shallow (stencil) products on the fused
 * reference-order kernel, of which whole general Horner steps res * subst + slab in one launch, two unused words (0),
 * one more unused word (0), recorded observation chains launched with the consumer's Add as their epilogue, linearity scans
 * answered by a proof about exact zeros (intervals), Adds that evaluated recorded sums in their own launch, executions of the
 * deferred launch graph, recordings issued through them, batched launches, items in them, microseconds of the calling thread
 * inside graph executions}.  Diagnostics; bench.py's e2e rows. */
size_t gft_op_stats_ex(size_t* out, size_t cap);
/* hipEvent timing on the library's stream: record into slot 0..63, elapsed in ms (syncs on b). */
int gft_event_record(int slot);
float gft_event_elapsed_ms(int slot_a, int slot_b);
/* Which convolution kernel `mul` may use: 0 = auto, 1 = force the simple one-thread-per-output
 * kernel, 2 = force the LDS-tiled FMA kernel (errors if the shape is unsupported), 3 = force the
 * LDS-staged reference-order kernel wherever its shape limits allow.  Modes 1 and 3 are bit-identical
 * to each other and to the CPU algorithm.  Test/bench knob. */
int gft_set_conv_mode(int mode);
/* Switches and thresholds by name (returns -1 for an unknown name).  README lists them with their environment variables.
 * SWITCHES (1 = on, the default; 0 = the simpler form, for A/B runs, bisecting and the verification matrix):
 *   "batch_dag"     recordings form a deferred launch graph that is issued level by level as batched launches
 *   "lazy_observe"  observation chains are recorded on their result instead of launched (and take the consumer's Add as epilogue)
 *   "lazy_sum"      Adds of two deferred chains are recorded (nested Adds evaluate them in one launch)
 *   "lazy_horner"   proven linear Horner loops are recorded (with "batch_dag")
 *   "nz_proofs"     interval Horner loops skip the linearity scan where the operand's exact zeros are proven to be none, or whole
 *                   leading slabs
 *   "defer"         elementwise operations are deferred into chains instead of launched one by one
 *   "async_launch"  kernels are issued by the library's launch thread instead of the calling thread
 *   "div_wavefront" division / log / exp recurrences as one-launch wavefronts (0: the slab-by-slab blocked form)
 *   "exp_right"     large f64 exponentials add their terms in arrival order (1e-10 contract; 0: the reference's order everywhere)
 *   "recur_overlap" the blocked recurrences overlap their bulk updates on a second stream (test knob: same bits either way)
 * THRESHOLDS: "host_max_elems" / "host_max_macs" (size-threshold dispatch: largest result, in elements, and largest general
 * product, in multiply-adds, computed on the host tier; 0 = everything on the device), "tiled_min_macs" (auto-mode crossover to
 * the tiled product), "horner_loop_max" (largest final tensor, in elements, whose linear Horner steps all run in one launch; 0 =
 * one launch per step), "shallow_max_terms" (plain products whose outputs receive at most this many terms run on the fused
 * reference-order kernel; 0: never; negative: the default, 256), "shallow_pair_min" (smallest result for which a flat stencil
 * computes two outputs per thread; -1: the default 4096, below: never), "conv_rb_min_macs" (smallest interval product on the
 * register-blocked rows kernel; negative: never), "conv_rb_pairs" (the reference-order product as row-pair sums: 0 never, 1 by
 * size, 2 whenever it applies, negative: the default), "conv_rb_pairs_cap" (bytes of row sums that form may hold at a time;
 * default 2 GiB), "conv_rb_pairs_lanes" (its slab ranges on two lanes: 0 never, 1 always, negative: the default rule),
 * "tiled_tile" (3..6 force the tiled product's lane tile 8x8 .. 1x64; 0: the planner's choice), "tiled_peel" (the peel of
 * the diagonal lane triangles of rank-3 products of full operands: -1 by size, 0 never, 1 wherever the structure allows;
 * gft_op_stats_ex slot 7 counts the peeled products), "tiled_peel_lanes" (0: a peeled product stays on one stream; 1: the
 * main kernels of its two leftover launches run on the library's two internal lanes beside the main part, joined before
 * their reduces — the same bits, and never while the stream is being captured; negative: the default, 1 where both leftover
 * launches have more ranges than the device has workgroup slots, 0 elsewhere; slot 8 counts the products that forked), "tiled_slots" (at most this many workgroups per main launch of the tiled
 * product, which then claim the plan's stream-K ranges; 0: the default, one per range or per resident slot; negative: one per
 * range, the static launch; never changes the cuts, so results do not depend on it), "tiled_taper" (how far the ranges of a
 * claiming plan taper along a queue, in per cent of their mean; negative: the default), "dist_min_macs" (smallest
 * general product gft_mul shards over the GPUs of gft_dist_init), "dist_event_slot", "series_form" (gft_series_last_form).
 * TEST KNOBS: "debug_fail_next_launch" (1: the next kernel launch requests 1 MB of LDS and fails — on the launch thread; the
 * failure is reported by the next gft_synchronize / value inspection), "trace_lq_report". */
int gft_set_option(const char* name, double value);
/* Tiled-kernel variant for A/B measurements (-1 = library default).  Test/bench knob. */
int gft_set_conv_variant(int variant);

/* ---- raw device-pointer entry points (no handles) ---------------------------------------- */
/* res[k] (+)= sum_j x[j]*y[k-j] for k0 in [slab_lo, slab_hi): the truncated N-d Cauchy product
 * `mul` of mt:984-1012 on caller-owned contiguous row-major device buffers (e.g. torch tensors),
 * restricted to a range of leading-axis output slabs — the unit of multi-GPU sharding and of the
 * div/exp/log recurrences.  accumulate=0 overwrites the slabs, 1 adds to them.  Runs on the
 * current stream; does not synchronise. */
int gft_conv_raw(const double* x, const size_t* xshape, const double* y, const size_t* yshape, double* res,
                 const size_t* rshape, size_t ndim, size_t slab_lo, size_t slab_hi, int accumulate);
/* Exact multiply-accumulate count of those slabs (sum_k prod_v #{valid j_v}). */
double gft_conv_macs(const size_t* xshape, const size_t* yshape, const size_t* rshape, size_t ndim,
                     size_t slab_lo, size_t slab_hi);
/* Leading-axis slab assignment for `world` ranks (work of slab k is proportional to the number
 * of valid j0, i.e. triangular): writes for `rank` up to 2 half-open ranges
 * {lo0,hi0,lo1,hi1} (folded: low group + mirrored high group).  Pure integer logic; needs no GPU.
 * Returns 1 if every rank's two groups have equal sizes (all-gather friendly), 0 otherwise. */
int gft_plan_slabs(size_t n0, int world, int rank, size_t out[4]);

/* ---- batched univariate series on caller-owned device tensors ------------------------------
 * B independent truncated power series per call.  The last axis of every operand is the series (coefficient k of t^k at
 * index k, UNIT stride), the `nbatch` leading axes of extents `batch` are the batch.  Item b of an operand is the
 * TaylorPoly<F64> of one variable with stored coefficients x[b, :nx] and degrees_p1 = (n); nx, ny <= n (a shorter operand
 * is compact: its high orders are implicit zeros, mt:13-19); the result has n coefficients per item, n <= 4096 in this
 * version.  `xbs` / `ybs` / `sbs` / `rbs` are the element strides of the batch axes (NULL = contiguous rows of the
 * operand's own length nx / ny / 1 / n).  Any non-negative stride on an input, 0 included (one series against the whole
 * batch); the result's rows must not overlap each other (no zero stride on an axis longer than 1) and the result may share
 * memory with an input only as the SAME view (in place) — any other overlap, judged by address ranges, is refused.  An
 * empty batch is a no-op.
 * Per item the result is the reference's GENERAL algorithm in its operation order, multiply and add rounded separately.
 * NONE of the data-dependent shortcuts of the operator wrappers is taken (Mul: zero / one / constant / linear operand,
 * mt:1020-1070; Div: divisor one / constant, mt:1204-1213): a batch cannot branch per item on the host, and the result of
 * an item never depends on what else is in the batch.  Coefficients the reference would leave unstored (beyond nx + ny - 1
 * of a product, beyond the first of exp / log of a one-coefficient operand) are written as +0.0.
 * exp / log: `seed` holds exp(x[b, 0]) / ln(x[b, 0]) per item (batch strides `sbs`); with the platform libm's values the
 * whole result carries the reference's bits.  seed == NULL forms the seeds on the device with the HIP device library's
 * exp / log, a few ulps from the host libm's (the other coefficients of log do not depend on the seed).
 * Stream contract: gft_from_device's — ordered after everything issued so far on `stream` and on the library's stream,
 * before everything issued later on either; the call does not wait.  0 on success, -1 with gft_last_error() otherwise. */
int gft_series_mul(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                   double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,
                   void* stream);                                       /* mul_1d                 mt:972-982   */
int gft_series_div(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                   double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,
                   void* stream);                                       /* div (one axis)         mt:1162-1192 */
int gft_series_exp(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs,
                   double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,
                   void* stream);                                       /* exp_1d                 mt:1271-1283 */
int gft_series_log(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs,
                   double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,
                   void* stream);                                       /* log_1d                 mt:1319-1333 */
/* compose: res[b] = f[b](g[b]) truncated at order n, f in the place of x and g in the place of y (nf, ng <= n).  Per item it is
 * subst_var's general Horner path (mt:574-578) with the general product mul_1d at every step and none of the shortcuts of
 * subst_var (zero / linear substitution, mt:547-568) or of Mul: res = [0.0 + f[nf-1]]; for i = nf-2 .. 0: res = res * g
 * truncated at the compact length min(len(res) + ng - 1, n) (sum_shape, mt:150-170), res[0] = res[0] + f[i]; the result is res
 * extended with +0.0 to n.  The whole loop of a series runs in one kernel with the row resident in LDS.  Cost: about
 * nf * n^2 / 2 multiply-adds per item, on one workgroup at most (no cap is imposed; nf = n = 4096 is 3.4e10 of them for one series).
 * pow: res[b] = x[b]^e by the reference's square-and-multiply (mt:441-450) over the same product and compact lengths
 * min(la + lb - 1, n): res = [1.0], base = x; while e > 0: if e & 1 then res = res * base; e >>= 1; if e > 0 then
 * base = base * base.  e == 0 gives [1, 0, ...]; e == 1 runs the loop (0.0 + 1.0 * x[k]: it differs from the reference's clone in
 * the sign of a zero).  A sequence of the batched mul launches on pool workspace inside the one stream-ordered call. */
int gft_series_compose(const double* f, const int64_t* fbs, size_t nf, const double* g, const int64_t* gbs, size_t ng,
                       double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch,
                       void* stream);                                   /* subst_var (Horner)     mt:540-580   */
int gft_series_pow(const double* x, const int64_t* xbs, size_t nx, uint32_t e, double* res, const int64_t* rbs, size_t n,
                   const size_t* batch, size_t nbatch, void* stream);   /* pow                    mt:433-451   */
/* corr: the transposed product, the adjoint of mul in the truncated inner product, <mul(x, y), g> = <x, corr(g, y)> (f64 only; no
 * gfti_ twin: a gradient of interval bounds is not defined).  g has ng <= 4096 coefficients, y has ny <= ng, the result m <= ng:
 *   res[i] = 0.0 + sum_k g[k] * y[k - i],   k DESCENDING from min(ng - 1, i + ny - 1) to i,   i = 0 .. m - 1,
 * multiply and add rounded separately, only stored operands entering a sum.  The descending order makes res[i] bit for bit
 * mul_1d(flip(g), y) at index ng - 1 - i in the reference's ascending order.  The result may be g itself (the same view, m == ng);
 * it may NOT overlap y (refused), and any other overlap is refused as for the other operations.
 * compose_adj: the transposed Horner loop, the gradient of compose(f, g, n) with respect to f.  gh has n coefficients (the gradient
 * of the composition), g has ng <= n, the result nf <= n.  With l_i = min(1 + (nf - 1 - i)(ng - 1), n), the compact lengths of the
 * forward loop: a_0 = gh[0 .. l_0); res[i] = a_i[0]; a_{i+1}[p] = 0.0 + sum_k a_i[k] * g[k - p], k DESCENDING from
 * min(l_i - 1, p + ng - 1) to p, p < l_{i+1} -- every step is corr at the compact lengths.  One kernel, one workgroup per series
 * (gft_series_last_form() == 2).  The result may be gh itself (the same view, nf == n); it may NOT overlap g (refused). */
int gft_series_corr(const double* g, const int64_t* gbs, size_t ng, const double* y, const int64_t* ybs, size_t ny,
                    double* res, const int64_t* rbs, size_t m, const size_t* batch, size_t nbatch,
                    void* stream);                                      /* mul_1d transposed                   */
int gft_series_compose_adj(const double* gh, const int64_t* hbs, size_t n, const double* g, const int64_t* gbs, size_t ng,
                           double* res, const int64_t* rbs, size_t nf, const size_t* batch, size_t nbatch,
                           void* stream);                               /* subst_var (Horner) transposed       */
/* The form the last gft_series_* call took: 1 = one lane per series (rows in LDS), 2 = one wave / workgroup per series (exp /
 * log: the lane-per-series loop over a transposed workspace; pow: the form of its last product), 0 = none yet.  gft_set_option("series_form", 1 | 2) asks for a
 * form (1 holds only where the rows fit the LDS budget; 0 = the library's thresholds).  Test / measurement aid. */
int gft_series_last_form(void);

/* ---- batched BIVARIATE series on caller-owned device tensors (f64 only): mul / div / exp / log / compose / pow ----
 * The last TWO axes of every operand are the coefficient array of one TaylorPoly<F64> in two variables: axis -2 is variable 0
 * (`nx0` rows, `xrs` elements apart: any non-negative stride), axis -1 is variable 1 (`nx1` coefficients, UNIT stride).  The
 * `nbatch` leading axes are the batch, with strides `xbs` / `ybs` / `sbs` / `rbs` as for gft_series_* (NULL = contiguous items
 * of the operand's own shape).  x has stored shape (nx0, nx1), y (ny0, ny1), the result always (n0, n1) with nx*, ny* <= n*,
 * n0, n1 >= 1 and n0 * n1 <= 4096 in this version.  The result's rows and items must be distinct addresses (its row stride
 * joins the batch strides in that proof); the result may be an operand itself (the same view), any other overlap is refused by
 * address range.  Per item the result is the reference's GENERAL recursion over axis 0 in its operation order, multiply and add
 * rounded separately, only stored coefficients entering a sum, and none of the operator wrappers' zero / one / constant /
 * linear shortcuts.  With mul1d / div1d / exp1d / log1d the loops of gft_series_* (sums from 0.0):
 *   mul  z = 0;  for k < n0, j ascending in max(0, k+1-ny0) .. min(k+1, nx0)-1:  z[k] += mul1d(x[j], y[k-j], n1)
 *        (the row sum is formed from 0.0 FIRST, then added to z[k])
 *   div  for k < n0:  c = 0;  for j in max(0, k+1-ny0) .. k-1: c += mul1d(r[j], y[k-j], n1);  c = -c;
 *        if k < nx0: c[:nx1] += x[k];  r[k] = div1d(c, y[0], n1)
 *   exp  r[0] = exp1d(x[0], n1, seed);  for k >= 1:  c = 0;  for j in 1 .. min(nx0, k+1)-1: c += mul1d(x[j] * (double)j, r[k-j], n1);
 *        r[k] = c / (double)k          (x[j] * j is rounded before it meets r)
 *   log  r[0] = log1d(x[0], n1, seed);  for k >= 1:  c = 0;  for j in max(1, k+1-nx0) .. k-1: c += mul1d(x[k-j], r[j] * (double)j, n1);
 *        c = -c;  if k < nx0: c[:nx1] += (double)k * x[k];  c = div1d(c, x[0], n1);  r[k] = c / (double)k
 * These are the bits of the reference's *, /, exp() and log() at rank 2 wherever the divisor / the operand of log stores at
 * least 2 coefficients on both axes; elsewhere (where the reference shortcuts or stores fewer rows) the loops are the
 * definition and differ from it in signs of zeros only.  `seed`: exp(x[b, 0, 0]) / ln(x[b, 0, 0]) per item, or NULL (formed on
 * the device), as for gft_series_exp / log.  One kernel per call, one workgroup per item with the operands resident in LDS;
 * where the runtime grants less LDS than an item needs the call fails and says so.  gft_series_last_form() reports 2 afterwards;
 * the "series_form" option does not apply.  Stream contract and return values: those of gft_series_*. */
int gft_series2_mul(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs,
                    int64_t yrs, size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1,
                    const size_t* batch, size_t nbatch, void* stream);   /* mul                    mt:984-1012  */
int gft_series2_div(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs,
                    int64_t yrs, size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1,
                    const size_t* batch, size_t nbatch, void* stream);   /* div                    mt:1162-1192 */
int gft_series2_exp(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs,
                    double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                    void* stream);                                       /* exp                    mt:1285-1317 */
int gft_series2_log(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs,
                    double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                    void* stream);                                       /* log                    mt:1335-1386 */
/* compose: res[b] = f[b] with g[b] substituted for variable `var` (0: the row axis, 1: the unit-stride axis) of f, f in the place
 * of x (stored shape (nf0, nf1)) and g in the place of y ((ng0, ng1)), truncated at (n0, n1).  With mul2(a, b, L) the loop of
 * gft_series2_mul on the stored shapes truncated at L, it is subst_var's general Horner path (mt:569-579) with the general product
 * at every step and none of the shortcuts of subst_var (mt:547-568) or of Mul.  var == 0:
 *   res = [[0.0 + f[nf0-1][c], c < nf1]]                           (stored shape (1, nf1))
 *   for i = nf0-2 .. 0:  L = (min(r0 + ng0 - 1, n0), min(r1 + ng1 - 1, n1)), (r0, r1) the stored shape of res (sum_shape);
 *                        res = mul2(res, g, L);  res[0][c] = res[0][c] + f[i][c], c < nf1
 * and the result is res extended with +0.0 to (n0, n1).  var == 1 is the same loop over the columns of f: res starts as the column
 * 0.0 + f[:, nf1-1], stored shape (nf0, 1), and after each product res[r][0] = res[r][0] + f[r][i], r < nf0.  With one slice
 * (nf0 == 1, resp. nf1 == 1) the result is 0.0 + f padded and g's values are not used.  A var other than 0 or 1 is refused.  One
 * kernel, one workgroup per item for the whole loop, the result resident in LDS from step to step (g beside it where the granted
 * LDS holds both, else read from global memory).  Cost: about nslices * (n0 * n1)^2 / 4 multiply-adds per item on that one
 * workgroup; no cap is imposed.  The result may be f or g itself (the same view).
 * pow: res[b] = x[b]^e by the reference's square-and-multiply (mt:433-451) without its wasted last squaring, over mul2 at the
 * compact shapes min(la + lb - 1, n) per axis: res = [[1.0]], base = x; while e > 0: if e & 1 then res = mul2(res, base);
 * e >>= 1; if e > 0 then base = mul2(base, base).  The result is padded with +0.0; e == 0 gives the unit item, e == 1 runs the
 * loop (0.0 + 1.0 * x).  A sequence of gft_series2_mul's launches on pool workspace inside the one stream-ordered call. */
int gft_series2_compose(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, const double* g, const int64_t* gbs,
                        int64_t grs, size_t ng0, size_t ng1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t n0,
                        size_t n1, const size_t* batch, size_t nbatch, void* stream);   /* subst_var (Horner)     mt:540-580   */
int gft_series2_pow(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, uint32_t e, double* res,
                    const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                    void* stream);                                       /* pow                    mt:433-451   */
/* ---- batched TRIVARIATE series on caller-owned device tensors (f64; gfti_series3_* below): mul / div / exp / log / compose / pow ----
 * The last THREE axes of every operand are the coefficient array of one TaylorPoly<F64> in three variables: axis -3 is variable 0
 * (`nx0` slabs, `xss` elements apart), axis -2 variable 1 (`nx1` rows, `xrs` elements apart) -- any non-negative strides -- and
 * axis -1 variable 2 (`nx2` coefficients, UNIT stride).  Per operand the arguments are the pointer, the batch-stride array, the
 * slab stride, the row stride and the three lengths; then the batch shape, nbatch and the stream.  x has stored shape
 * (nx0, nx1, nx2), y (ny0, ny1, ny2), the result always (n0, n1, n2) with nx*, ny* <= n*, n* >= 1 and n0 * n1 * n2 <= 4096 in this
 * version.  The result's slabs, rows and items must be distinct addresses (its slab stride joins the row and batch strides in
 * that proof); the result may be an operand itself (the same view), any other overlap is refused by address range.  Per item the
 * result is the reference's GENERAL recursion over axis 0 in its operation order, multiply and add rounded separately, only stored
 * coefficients entering a sum, and none of the operator wrappers' zero / one / constant / linear shortcuts.  Two rules, both
 * decided by the shapes alone and so the same for every item of a call, come before the loops:
 *   1. The recursion runs on the STORED RESULT SHAPE S, not on n.  Per axis a:
 *        mul        S_a = min(n_a, nx_a + ny_a - 1)                    (sum_shape, mt:150-170)
 *        div        S_a = n_a, except S_a = nx_a where ny_a == 1       (mt:1216-1221)
 *        exp, log   S_a = n_a, except S_a = 1 where nx_a == 1          (mt:408-413, 421-426)
 *      Every coefficient of the result outside S is +0.0.
 *   2. The unit axes of S are SQUEEZED: an item whose S has one axis of length 1 is by definition the gft_series2_* item without
 *      that axis (its loops above, on the two remaining axes in their order), with two such axes the gft_series_* row, with three
 *      the same loops at one coefficient.  (The reference forms a whole 1-d product from 0.0 before it adds it, so the loops
 *      below, run over an axis of length 1, would associate differently.)
 * With every S_a >= 2, mul1d the univariate product of gft_series_mul at S_2 coefficients (a sum from 0.0) and div2 / exp2 / log2
 * the loops of gft_series2_div / exp / log at (S_1, S_2):
 *   mul  for k0 < S_0:  z[k0] = 0;  for j0 ascending in max(0, k0+1-ny0) .. min(k0+1, nx0)-1, and for every row k1 < S_1, for j1
 *        ascending in max(0, k1+1-ny1) .. min(k1+1, nx1)-1:  z[k0][k1] += mul1d(x[j0][j1], y[k0-j0][k1-j1])
 *        (one accumulator per row (k0, k1); each mul1d is formed from 0.0 FIRST, then added).  Written a (*) b for two slabs below.
 *   div  for k0 < S_0:  c = 0;  for j0 in max(0, k0+1-ny0) .. k0-1: c += r[j0] (*) y[k0-j0];  c = -c;
 *        if k0 < nx0: c[:nx1][:nx2] += x[k0];  r[k0] = div2(c, y[0])
 *   exp  r[0] = exp2(x[0], seed);  for k0 >= 1:  c = 0;  for j0 in 1 .. min(nx0, k0+1)-1: c += (x[j0] * (double)j0) (*) r[k0-j0];
 *        r[k0] = c / (double)k0          (x[j0] * j0 is rounded before it meets r)
 *   log  r[0] = log2(x[0], seed);  for k0 >= 1:  c = 0;  for j0 in max(1, k0+1-nx0) .. k0-1: c += x[k0-j0] (*) (r[j0] * (double)j0);
 *        c = -c;  if k0 < nx0: c[:nx1][:nx2] += (double)k0 * x[k0];  c = div2(c, x[0]);  r[k0] = c / (double)k0
 * These are the bits of the reference's general product (mul) and of its /, exp() and log() at rank 3 wherever those take no
 * data-dependent shortcut; the one shortcut the shapes trigger is a divisor of ONE stored coefficient, where the loops are the
 * definition.  `seed`: exp(x[b, 0, 0, 0]) / ln(x[b, 0, 0, 0]) per item, or NULL (formed on the device), as for gft_series_exp /
 * log.  One kernel per call, one workgroup per item with the operands resident in LDS; where the runtime grants less LDS than an
 * item needs the call fails and says so.  gft_series_last_form() reports 2 afterwards; the "series_form" option does not apply.
 * Stream contract, NULL stride arrays, empty batches and return values: those of gft_series2_mul. */
int gft_series3_mul(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* y,
                    const int64_t* ybs, int64_t yss, int64_t yrs, size_t ny0, size_t ny1, size_t ny2, double* res, const int64_t* rbs,
                    int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch,
                    void* stream);                                       /* mul                    mt:984-1012  */
int gft_series3_div(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* y,
                    const int64_t* ybs, int64_t yss, int64_t yrs, size_t ny0, size_t ny1, size_t ny2, double* res, const int64_t* rbs,
                    int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch,
                    void* stream);                                       /* div                    mt:1162-1192 */
int gft_series3_exp(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* seed,
                    const int64_t* sbs, double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2,
                    const size_t* batch, size_t nbatch, void* stream);   /* exp                    mt:1285-1317 */
int gft_series3_log(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* seed,
                    const int64_t* sbs, double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2,
                    const size_t* batch, size_t nbatch, void* stream);   /* log                    mt:1335-1386 */
/* compose at rank 3: res[b] = f[b] with g[b] substituted for variable `var` of f (0: the slab axis, 1: the row axis, 2: the unit-stride
 * axis; anything else is refused), f in the place of x (stored shape nf = (nf0, nf1, nf2)) and g in the place of y (ng), truncated at
 * n = (n0, n1, n2) with nf, ng <= n per axis and n0 * n1 * n2 <= 4096.  With mul3(a, b, L) gft_series3_mul on the stored shapes of a and
 * b truncated at L -- BOTH of its rules: computed on S = min(L, na + nb - 1), the unit axes of S squeezed -- it is subst_var's general
 * Horner path (mt:569-579) with none of the shortcuts of subst_var (mt:547-568) or of Mul.  The slices of f are taken along axis var:
 *   res = 0.0 + the last slice                                     (stored shape r: nf with 1 on axis var)
 *   for i = nf[var]-2 .. 0:  L_a = min(r_a + ng_a - 1, n_a) per axis, r the stored shape of res (sum_shape);  res = mul3(res, g, L);
 *                            slice i is added into res[... index 0 on axis var ...] over the slice's stored extent, one addition per
 *                            coefficient
 * and the result is res extended with +0.0 to n.  With one slice the result is 0.0 + f padded and g's values are not read.  L_a == 1
 * holds iff n_a == 1, or ng_a == 1 and res started with 1 on the axis (a == var, or nf_a == 1), so the set of squeezed axes is the same
 * for every step of a call and is that of the final stored shape.  One kernel, one workgroup per item for the whole loop, the result
 * resident in LDS from step to step (g beside it where the granted LDS holds both, else read from global memory).  Cost: about
 * nf[var] * (n0 * n1 * n2)^2 / 8 multiply-adds per item on that one workgroup; no cap is imposed.  The result may be f or g itself (the
 * same view); any partial overlap is refused.
 * pow at rank 3: res[b] = x[b]^e for 0 <= e < 2^32 by the reference's square-and-multiply (mt:433-451) without its wasted last squaring,
 * over mul3 at the compact shapes min(la + lb - 1, n) per axis: res = [[[1.0]]], base = x; while e > 0: if e & 1 then res = mul3(res,
 * base); e >>= 1; if e > 0 then base = mul3(base, base).  The result is padded with +0.0; e == 0 gives the unit item, e == 1 runs the
 * loop (0.0 + 1.0 * x, so -0.0 becomes +0.0).  A sequence of gft_series3_mul's launches on pool workspace (3 * items * n0 * n1 * n2 + 1
 * doubles) inside the one stream-ordered call, no host synchronisation; the result may be x itself.  A batch with more than 10
 * non-contiguous axes is refused.  gft_series_last_form() reports 2 after either. */
int gft_series3_compose(const double* f, const int64_t* fbs, int64_t fss, int64_t frs, size_t nf0, size_t nf1, size_t nf2, const double* g,
                        const int64_t* gbs, int64_t gss, int64_t grs, size_t ng0, size_t ng1, size_t ng2, int var, double* res,
                        const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch,
                        void* stream);                                   /* subst_var (Horner)     mt:540-580   */
int gft_series3_pow(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, uint32_t e,
                    double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch,
                    size_t nbatch, void* stream);                        /* pow                    mt:433-451   */
/* corr at rank 2: the transposed product, the adjoint of gft_series2_mul in the truncated inner product,
 * <mul2(x, y, (g0, g1)), g> = <x, corr2(g, y)> (f64 only; no gfti_ twin, for the reason given at gft_series_corr: a gradient of
 * interval bounds is not defined).  g has stored shape (g0, g1) with g0 * g1 <= 4096, y has (ny0, ny1) <= (g0, g1) per axis, the
 * result (m0, m1) <= (g0, g1) per axis:
 *   res[i0][i1] = 0.0 + sum over k0 DESCENDING from min(g0-1, i0+ny0-1) to i0 of
 *                 (0.0 + sum over k1 DESCENDING from min(g1-1, i1+ny1-1) to i1 of g[k0][k1] * y[k0-i0][k1-i1])
 * multiply and add rounded separately, only stored coefficients entering a sum; the inner row sum is formed from 0.0 FIRST and then
 * added to the outer one.  That order makes res[i0][i1] bit for bit mul2(flip(g), y, (g0, g1))[g0-1-i0][g1-1-i1], flip reversing both
 * series axes.  One kernel, one workgroup per item, g and y resident in LDS.  Aliasing: the result may be g itself as the SAME view
 * (then m == g); it may NOT overlap y, and any partial overlap with g is refused by address range as for the other entries.
 * compose_adj at rank 2: the transposed Horner loop, the gradient of gft_series2_compose(f, g, var, (n0, n1)) with respect to f.  gh
 * has shape (n0, n1) (the gradient of the composition), g has (ng0, ng1) <= n, the result f's stored shape (nf0, nf1) <= n; var is 0 or
 * 1, anything else is refused.  Let S be the number of slices of f and len their length (S = nf0, len = nf1 for var 0, the other way
 * round for var 1), base = (1, len) for var 0 and (len, 1) for var 1, and L_i[a] = min(base[a] + (S-1-i) * (ng_a - 1), n_a), i < S, the
 * compact shapes of the forward loop.  Then a_0 = gh[:L_0[0], :L_0[1]]; slice i of the result is the first len entries of row 0
 * (var 0) or column 0 (var 1) of a_i; a_{i+1} = corr2(a_i, g) at the result shape L_{i+1} -- every step is the sum above at the compact
 * shapes.  One kernel, one workgroup per item for the whole loop, a resident in LDS (g beside it where the granted LDS holds both,
 * else read from global memory).  With one slice the result is gh's leading entries and g's values are not read.  The result may be
 * gh itself as the same view; it may NOT overlap g (refused).
 * Argument conventions, stream contract, empty-batch behaviour and return values of both: those of gft_series2_mul. */
int gft_series2_corr(const double* g, const int64_t* gbs, int64_t grs, size_t g0, size_t g1, const double* y, const int64_t* ybs,
                     int64_t yrs, size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t m0, size_t m1,
                     const size_t* batch, size_t nbatch, void* stream);  /* mul transposed                      */
int gft_series2_compose_adj(const double* gh, const int64_t* hbs, int64_t hrs, size_t n0, size_t n1, const double* g, const int64_t* gbs,
                            int64_t grs, size_t ng0, size_t ng1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t nf0,
                            size_t nf1, const size_t* batch, size_t nbatch, void* stream);   /* subst_var (Horner) transposed */

/* ---- batched observation ops on caller-owned device tensors: derivative / taylor_expansion_of_coeff / shift_down /
 * evaluate_all_one at ranks 1 (gft_series_*) and 2 (gft_series2_*), what `observe X = k`, `X -= k` and the mass read-outs are made
 * of.  One operand x of stored length nx (rank 2: shape (nx0, nx1), rows xrs elements apart) per item; `k` is the order, at rank 2
 * behind `var`, the axis it acts on (0: axis -2, 1: axis -1).  0 <= k < the stored length on that axis, anything else is refused
 * before the device is touched.  The result has the operand's shape with k taken off that axis, and (n | n0, n1) must say so.
 * Batch strides, row strides, NULL stride arrays, empty batches, the stream contract and return values: those of gft_series_mul /
 * gft_series2_mul; the limits nx <= 4096 and nx0 * nx1 <= 4096 bound the OPERAND.  The result may be x itself as the same view
 * (possible at k == 0 only); every other overlap is refused.  Per item, with T::from_u32 the conversion and every operation rounded
 * once, the loops along the axis (the other index, if any, carried along) are the handle operations' (mt:457-536):
 *   derivative:                 out[j] = x[k + j] * ff_j;   ff_0 = ((1 * 1) * 2) ... * k,  ff_{j+1} = ff_j * (from(k + j + 1) / from(j + 1))
 *   taylor_expansion_of_coeff:  out[0] = x[k];  out[j] = x[k + j] * f_j, j >= 1;   f_0 = 1,  f_j = f_{j-1} * (from(k + j) / from(j))
 *   shift_down:                 out[0] = x[k] + S,  S the ordered sum of x[0 .. k) from 0.0;  out[j] = x[k + j], j >= 1;
 *                               when the stored length is k + 1, out[0] is the ordered sum of ALL its slices instead
 *   evaluate_all_one:           res = 0.0 + x[0] + x[1] + ... over the item in row-major order, one chain (mt:583-586); the result
 *                               has the batch shape, strides rbs
 * The quotient of a factor is rounded first, then the product: the factors are not the integers one would guess, and they depend on
 * (operation, k, length) only, so they are computed once by the handle path's table functor and cached.  The order of S is ndarray's
 * sum_axis: at rank 1 ascending; at rank 2 along axis 0 ascending over the rows, per column -- unless nx1 == 1, which, like every
 * sum along axis 1, is the 8-way unrolled fold: eight partial sums p_u over whole groups of eight (p_u += x[8 g + u]), then
 * (((0.0 + (p0 + p4)) + (p1 + p5)) + (p2 + p6)) + (p3 + p7), then the tail in order.  The additions of 0.0 are real: with k == 0
 * out[0] = x[0] + 0.0, and -0.0 becomes +0.0.  No data-dependent shortcut is taken.  One launch per call, no workspace;
 * gft_series_last_form() reports 0 afterwards. */
int gft_series_derivative(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,
                          const size_t* batch, size_t nbatch, void* stream);
int gft_series_taylor_expansion_of_coeff(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs,
                                         size_t n, const size_t* batch, size_t nbatch, void* stream);
int gft_series_shift_down(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,
                          const size_t* batch, size_t nbatch, void* stream);
int gft_series_evaluate_all_one(const double* x, const int64_t* xbs, size_t nx, double* res, const int64_t* rbs, const size_t* batch,
                                size_t nbatch, void* stream);
int gft_series2_derivative(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,
                           const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gft_series2_taylor_expansion_of_coeff(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k,
                                          double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,
                                          size_t nbatch, void* stream);
int gft_series2_shift_down(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,
                           const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gft_series2_evaluate_all_one(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, double* res,
                                 const int64_t* rbs, const size_t* batch, size_t nbatch, void* stream);

/* ---- batched fused Poisson observation chains: what `observe k ~ Poisson(lambda * X)` runs (generating_function.rs:678-711), per
 * item and in one launch -- gft_observe_chain's unfolding on caller-owned device tensors, at ranks 1 and 2.  nsteps steps; step t runs
 * at degree d_t = degree_p1 + (nsteps - 1 - t) with the constant cs[t]:
 *   discrete rate (x given):     (derivative(v, 1).truncate_to_degree_p1(d_t) * var(v, x, d_t)) * from(cs[t])
 *   continuous rate (x == NULL):  derivative(v, 1).truncate_to_degree_p1(d_t) * from(cs[t])
 * Every item has its own scalars: x has the batch shape (strides xbs), cs is [B..., nsteps] with unit stride on its last axis (batch
 * strides cbs); both may repeat through stride 0.  An item is a set of independent lines along the acted-on axis v (rank 1: the
 * series; rank 2: `var`, 0 is axis -2 and 1 is axis -1); every other axis is cut to min(len, d_t) at step t and carried along.  Per
 * line, with src the previous step's output (the operand at t = 0), L its length, dl = min(L - 1, d_t), and ff the derivative's
 * factors of order 1 (ff_0 = 1 * 1, ff_{j+1} = ff_j * (from(j + 2) / from(j + 1)), the quotient rounded first), every operation
 * rounded once and nothing contracted:
 *   D[j] = src[j + 1] * ff_j,  j < dl                                  (derivative, mt:471-479)
 *   discrete form, lout = min(dl + 1, d_t), for kv < lout:
 *       c == 0:  res = +0.0                                            (Mul's zero shortcut; the item is all +0.0 from here on)
 *       x == 0:  res = kv == 0 ? +0.0 : D[kv - 1] * 1                  (mul_var alone, mt:619-621)
 *       else:    A = (1 <= kv <= dl) ? D[kv - 1] * 1 : +0.0;  res = 0.0 + A;
 *                if kv < dl:  res = res + (x == 1 ? D[kv] : x * D[kv])
 *       if c != 1:  res = c * res
 *   continuous form, lout = dl, for kv < lout:
 *       res = (c == 0) ? +0.0 : (c == 1 ? D[kv] : c * D[kv])
 * `==` compares values (-0.0 counts as zero).  The three tests of the scalars are made per item on the device and are the only
 * data-dependent branches; non-finite scalars and data run the same sequence, and no shortcut looks at the coefficients.
 * Shape rules, refused by name before the device is touched: degree_p1 >= 2, nsteps >= 1, degree_p1 + nsteps <= L_0 (the operand's
 * stored length on v), so every step is full: dl == lout == d_t.  The result has degree_p1 coefficients on v and min(len, degree_p1)
 * on the other axis of a rank-2 item, and (n | n0, n1) must say so.  The limits bound the operand (na <= 4096, na0 * na1 <= 4096).
 * The result may not overlap a, x or cs.  Batch strides, row strides, NULL stride arrays, empty batches, the stream contract and
 * return values: those of gft_series_mul.  One launch per call, no workspace; gft_series_last_form() reports 1 (one wave per line:
 * L_0 <= 64) or 2 (one workgroup per line), and the option "series_form" forces 2. */
int gft_series_observe_chain(const double* a, const int64_t* abs, size_t na, const double* x, const int64_t* xbs, const double* cs,
                             const int64_t* cbs, size_t nsteps, size_t degree_p1, double* res, const int64_t* rbs, size_t n,
                             const size_t* batch, size_t nbatch, void* stream);
int gft_series2_observe_chain(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* x,
                              const int64_t* xbs, const double* cs, const int64_t* cbs, size_t nsteps, size_t degree_p1, double* res,
                              const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);

/* ---- batched fused negative-binomial observation: what `observe k ~ NegBinomial(X, p)` runs (generating_function.rs:712-751), per
 * item and in one launch each: the row of scaled Lah numbers, and the sum over it.
 *
 * gft_series_lah_row: p has the batch shape (strides pbs, stride 0 allowed), the result is [B..., order + 1] (unit stride on its last
 * axis, batch strides rbs).  row_0 = [1];  for d = 1 .. order, i = 0 .. d:
 *       row_d[i] = ((1 - p) / from(d)) * (row_{d-1}[i] * from(d + i - 1) + row_{d-1}[i - 1])
 * where an entry row_{d-1} does not have is zero -- and is multiplied by and added all the same (-0.0, intervals).  order + 1 <= 4096.
 * The result may not overlap p.  gft_series_last_form(): 1 (one wave per item: order + 1 <= 64) or 2 (one workgroup per item).
 *
 * gft_series_observe_negbinomial / gft_series2_observe_negbinomial: a is the inner generating function evaluated at p * x to
 * degree_p1 + K coefficients on the acted-on axis v (rank 1: the series; rank 2: `var`), x and p one scalar per item each (strides
 * xbs, pbs), ls [B..., nls] the row, nls = K + 1 (unit stride on its last axis, batch strides lbs; usually gft_series_lah_row(p, K),
 * but any row).  With d = degree_p1 and L the stored length on v, per item:
 *   c = p * x, m = p * 1 -- but c = x, m = 1 where p == 1                     (from(p) * var(v, x, d): Mul returns var itself)
 *   pf[0] = 1, pf[j + 1] = pf[j] * m                                          (subst_var's power table, mt:555-567)
 *   P_1 = [c, m];  P_{i+1} = mul_linear(P_i, c, m) at length min(d, i + 2)    (gft_series_mul_linear's loops)
 * and per line along v (of a rank-2 item the first min(other axis, d) lines), D_0 = a[0 .. d + K):
 *   for i = 0 .. K:
 *       S[j] = D_i[j] * pf[j],  j < d
 *       i == 0:  U = S;   i == 1:  U = mul_linear(S, c, m) at length d
 *       i >= 2:  U[j] = 0 + (((0 + S[lo] * P_i[j - lo]) + ...) + S[j] * P_i[0]),  lo = max(0, j + 1 - len P_i)   (mul_1d, mt:971-982)
 *                -- but where the lines are the columns of a rank-2 item with more than one line the product walks the rows, every
 *                term passes through a sum of its own:  U[j] = ((0 + (0 + S[lo] * P_i[j - lo])) + ...) + (0 + S[j] * P_i[0])
 *       V = ls[i] == 1 ? U : ls[i] * U;   ls[i] == 0:  V is the one-coefficient zero
 *       i == 0:  sum = V (all +0.0 for the zero), then sum[first] = sum[first] + 0 on the item's first element
 *       i >= 1:  sum[j] = (0 + sum[j]) + V[j];  against the zero only sum[first] = sum[first] + 0
 *       D_{i+1}[j] = D_i[j + 1] * ff_j                                        (derivative, the chain's ff; not after the last pass)
 * `==` compares values (-0.0 counts as zero; an interval equals 0 or 1 when both bounds do).  The tests of p, c and ls[i] are made per
 * item on the device and are the only data-dependent branches; no shortcut looks at the coefficients.
 * Shape rules, refused by name before the device is touched, in this order: nls >= 1, degree_p1 >= 3, degree_p1 + K <= L,
 * 3 * degree_p1 + K <= 8192, and the result's shape: degree_p1 coefficients on v and min(len, degree_p1) on the other axis of a rank-2
 * item.  The limits bound the operand (na <= 4096, na0 * na1 <= 4096).  The result may not overlap a, x, p or ls.  Strides, empty
 * batches, the stream contract and return values: those of gft_series_mul.  One launch per call, no workspace;
 * gft_series_last_form() reports 1 (one wave per line: degree_p1 + K <= 64) or 2 (one workgroup per line), "series_form" forces 2. */
int gft_series_lah_row(const double* p, const int64_t* pbs, size_t order, double* res, const int64_t* rbs, const size_t* batch, size_t nbatch,
                       void* stream);
int gft_series_observe_negbinomial(const double* a, const int64_t* abs, size_t na, const double* x, const int64_t* xbs, const double* p,
                                   const int64_t* pbs, const double* ls, const int64_t* lbs, size_t nls, size_t degree_p1, double* res,
                                   const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gft_series2_observe_negbinomial(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* x,
                                    const int64_t* xbs, const double* p, const int64_t* pbs, const double* ls, const int64_t* lbs, size_t nls,
                                    size_t degree_p1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,
                                    size_t nbatch, void* stream);

/* ---- batched affine substitutions: what the reference runs wherever a series is multiplied by, or a variable replaced with, the
 * affine series c + m * x_w (X ~ Binomial(Y, p), X += Y, thinning, marginalising to a point, a Taylor shift) -- mul_linear
 * (mt:611-623) and subst_var's two linear paths (mt:555-579) on caller-owned device tensors, per item and in one launch, at ranks 1
 * and 2.  Every item has its own scalars: c and m have the batch shape (strides cbs, mbs) and may repeat through stride 0.  Axes are
 * counted as `var`: 0 is axis -2 and 1 is axis -1 of a rank-2 item; at rank 1 there is the series axis alone.  An operand lies inside
 * the orders (na <= n, per axis), the result has (n | n0, n1) coefficients, at least two on the axis w of the affine series, and the
 * limits bound the result (n <= 4096, n0 * n1 <= 4096).  Every operation is rounded once, nothing is contracted, and an absent term
 * is absent, not an added zero.
 *   mul_linear(a, c, m; w; n), a with L stored coefficients on w.  The compact result has L' = min(n_w, L + 1) on w and a's lengths
 *   on the other axis; per line along w:
 *       t[0] = +0.0,  t[j] = a[j - 1] * m                              1 <= j < L'      (mul_var, mt:589-608)
 *       c == 0:  out[j] = t[j]
 *       else:    out[j] = t[j] + (c * a[j])  for j < L,  out[L] = t[L] where L < L'
 *   and everything of n outside the compact result is +0.0.
 *   compose_linear(f, v, c, m, w; n): x_v := c + m * x_w.  S_i is slice i of f along v (i < nf_v).
 *       w == v and c == 0:  out slice i = S_i * p_i,  p_0 = 1,  p_{i+1} = p_i * m          (the running power table, mt:557-565)
 *       else:  res = 0.0 + S_{nf_v - 1};  for i = nf_v - 2 ... 0:                          (Horner, mt:569-579)
 *                  res = mul_linear(res, c, m; w; n) at its compact shape;  res[k] = res[k] + S_i[k] over the stored positions of S_i
 *   The result is res inside +0.0 at the orders n; for w != v only index 0 along v is ever stored.  The compact shape: f's for
 *   w == v; else 1 on v and min(n_w, nf_w + nf_v - 1) on w.
 * `c == 0` compares the value (-0.0 counts as zero), per item on the device: the only data-dependent branch.  Non-finite scalars
 * and data run the same sequence and no shortcut looks at the coefficients; gft_series_compose(f, [c, m]) is the general product's
 * operation order, other bits, and about nf * n^2 / 2 multiply-adds per item where this is nf * n.
 * The result may not overlap the operand, c or m (not even as the same view).  Batch strides, row strides, NULL stride arrays, empty
 * batches, the stream contract and return values: those of gft_series_mul.  One launch per call, no workspace.  After
 * compose_linear gft_series_last_form() reports 1 (one wave per line along w: n_w <= 64) or 2 (one workgroup per line), and the
 * option "series_form" forces 2; mul_linear is one streaming kernel and reports 0. */
int gft_series_mul_linear(const double* a, const int64_t* abs, size_t na, const double* c, const int64_t* cbs, const double* m,
                          const int64_t* mbs, double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gft_series2_mul_linear(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* c,
                           const int64_t* cbs, const double* m, const int64_t* mbs, double* res, const int64_t* rbs, int64_t rrs, size_t n0,
                           size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gft_series_compose_linear(const double* f, const int64_t* fbs, size_t nf, const double* c, const int64_t* cbs, const double* m,
                              const int64_t* mbs, double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gft_series2_compose_linear(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, int var, int wvar, const double* c,
                               const int64_t* cbs, const double* m, const int64_t* mbs, double* res, const int64_t* rbs, int64_t rrs, size_t n0,
                               size_t n1, const size_t* batch, size_t nbatch, void* stream);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI, collectives internal to the library --------
 * The reference is single-process; a host that wants one large product spread over the GPUs of a node starts one
 * process per GPU (each with its own gft_init(device)), lets rank 0 call gft_dist_unique_id, hands the 128 bytes to
 * the other ranks by whatever means it has (MPI, torch.distributed, a file), and has every rank call gft_dist_init.
 * From then on every rank runs the SAME program on replicated data; gft_mul shards a general f64 product of at least
 * "dist_min_macs" multiply-adds (gft_set_option, default 1e10) over the leading output axis — slab k depends on
 * x[0..=k], y[0..=k] and on no other output (mt:1001-1011), so there is no reduction: folded slab assignment
 * (gft_plan_slabs), local kernels, then in-place ncclAllGather of the low groups and grouped ncclSend/ncclRecv of the
 * mirrored high groups (zero-filled ncclAllReduce when the axis does not divide evenly) on the library's stream.
 * RCCL is dlopen'ed by gft_dist_init; single-GPU users never load it. */
int gft_dist_unique_id(void* out128);                                   /* ncclGetUniqueId (rank 0) */
int gft_dist_init(int rank, int world, const void* unique_id128);       /* ncclCommInitRank on the gft_init device */
int gft_dist_world(void);
int gft_dist_rank(void);
int gft_dist_comm_count(void);                                          /* ncclCommCount of the communicator (0: none) */
int gft_dist_shutdown(void);
/* Every rank (collective): small sharded products through both sharded entries — even split (all-gather + point-to-point)
 * and uneven split (zero-filled all-reduce) — against the rank's own full product, bit for bit.  0 = the exchange
 * delivers every slab; run automatically by gft_dist_init when GFT_DIST_SELFTEST=1 is in the environment. */
int gft_dist_selftest(void);
/* ncclBroadcast of `count` doubles at `buf` (device memory) from `root`: replicating operands that originate on one rank */
int gft_dist_broadcast(double* buf, size_t count, int root);
/* res = x (*) y like gft_conv_raw over ALL leading slabs, sharded over the communicator; x, y replicated on every rank,
 * every rank receives the full result.  With world == 1 (or before gft_dist_init) it is the plain product. */
int gft_conv_raw_sharded(const double* x, const size_t* xshape, const double* y, const size_t* yshape, double* res,
                         const size_t* rshape, size_t ndim);

/* ---- constructors ------------------------------------------------------------------------- */
gft_poly* gft_from_host(const double* coeffs, const size_t* shape, const size_t* degrees_p1,
                        size_t ndim);                                   /* TaylorPoly::new        mt:33-41   */
/* Copy a caller-owned DEVICE tensor into a new handle (TaylorPoly::new, mt:33-46; the handle owns a copy in its own pool
 * block).  `strides` are element strides (not bytes), ndim of them for gft_, ndim + 1 for gfti_ (the first is the lo -> hi
 * plane stride: interval data stacked as [2, *shape]); NULL = C-contiguous with the planes back to back, the gft_to_host
 * layout.  Stride 0 (a broadcast view) is accepted, negative strides are not.  `src` must be device memory of the library's
 * GPU.  Shape and degrees are validated as gft_from_host validates them.  Nothing is read on the host: the result is a
 * plain device tensor (no host tier, no affine shortcut).
 * Stream contract: `stream` is the caller's hipStream_t (0 = the HIP null stream, which is torch's default stream on
 * ROCm).  The copy is ordered after all work issued so far on the caller's stream and the library's, and before all work
 * issued later on either; the call does not wait for the copy.  `src` may be freed and reused on the caller's stream as
 * soon as the call returns. */
gft_poly* gft_from_device(const double* src, const int64_t* strides, const size_t* shape, const size_t* degrees_p1,
                          size_t ndim, void* stream);
gft_poly* gft_scalar(const double* x);                                  /* From<T>                mt:626-630 */
gft_poly* gft_from_u32(uint32_t c);                                     /* from_u32               mt:219-225 */
gft_poly* gft_zero_with(const size_t* degrees_p1, size_t ndim);         /* zero_with              mt:208-216 */
gft_poly* gft_var(size_t v, const double* x, size_t len);               /* var                    mt:239-248 */
gft_poly* gft_var_at_zero(size_t v, size_t len);                        /* var_at_zero            mt:228-237 */
gft_poly* gft_var_with_degrees_p1(size_t v, const double* x, const size_t* degrees_p1,
                                  size_t ndim);                         /* var_with_degrees_p1    mt:250-259 */
gft_poly* gft_clone(const gft_poly* p);                                 /* Clone                  mt:10      */
void gft_free(gft_poly* p);                                             /* Drop                              */

/* ---- queries ------------------------------------------------------------------------------ */
int gft_width(void);                                                    /* 1 (gfti_width() = 2)              */
size_t gft_num_vars(const gft_poly* p);                                 /* num_vars               mt:48-51   */
size_t gft_numel(const gft_poly* p);                                    /* coeffs.len()                      */
void gft_shape(const gft_poly* p, size_t* out);                         /* coeffs.shape() (compact)          */
void gft_degrees_p1(const gft_poly* p, size_t* out);                    /* shape()                mt:53-56   */
int gft_to_host(const gft_poly* p, double* out);                        /* array()/into_array     mt:58-66   */
/* Write the handle's coefficients, in its compact shape as gft_to_host gives them, into caller-owned DEVICE memory with the
 * given element strides (NULL = C-contiguous, planes back to back; gfti_ takes the plane stride first).  Zero strides on an
 * axis longer than 1, negative strides and destinations whose elements overlap are refused.  Lazy scalars, host-tier
 * tensors, deferred chains and recorded launch graphs are materialised on the device first.  Same stream contract as
 * gft_from_device: ordered after earlier work on both streams (torch kernels still reading or writing `dst` included),
 * before later work on both; 0 on success. */
int gft_to_device(const gft_poly* p, double* dst, const int64_t* strides, void* stream);
size_t gft_len_of(const gft_poly* p, size_t v);                         /* len_of                 mt:72-79   */
int gft_is_constant(const gft_poly* p);                                 /* is_constant            mt:68-70   */
int gft_is_zero(const gft_poly* p);                                     /* Zero::is_zero          mt:643-645 */
int gft_is_one(const gft_poly* p);                                      /* One::is_one            mt:653-655 */
int gft_equal(const gft_poly* a, const gft_poly* b);                    /* PartialEq              mt:10      */
/* Display (debug == 0: fmt_polynomial, mt:694-730, e.g. "1.0 + 2.0b + 3.0a^2") or Debug (debug != 0: "TaylorPoly([degrees_p1],
 * <polynomial>)", mt:632-636) as NUL-terminated UTF-8 into out[0..cap); returns the full length (call with cap 0 to size
 * the buffer), -1 on error.  Floats print like the reference's F64 (ryu shortest round-trip, f64.rs:41-45). */
long gft_format(const gft_poly* p, int debug, char* out, size_t cap);   /* Display / Debug        mt:632-636,694-730 */
int gft_constant_term(const gft_poly* p, double* out);                  /* constant_term          mt:296-299 */
int gft_extract_constant(const gft_poly* p, double* out);               /* extract_constant       mt:262-269 */
int gft_extract_linear(const gft_poly* p, double* c, double* m, size_t* v); /* extract_linear     mt:275-294 */
int gft_coefficient(const gft_poly* p, const size_t* index, size_t n, double* out); /* coefficient mt:314-339 */

/* ---- algebra ------------------------------------------------------------------------------ */
gft_poly* gft_add(const gft_poly* a, const gft_poly* b);                /* Add                    mt:854-882 */
gft_poly* gft_sub(const gft_poly* a, const gft_poly* b);                /* Sub                    mt:911-937 */
/* a + b * from(c) in one pass (the accumulation `sum += term * TaylorPoly::from(lah)` of the negative-binomial
 * observation, generating_function.rs:743-746): per element (0 + a) + (c * b), same operations and order as the two calls. */
gft_poly* gft_add_scaled(const gft_poly* a, const gft_poly* b, const double* c);
gft_poly* gft_neg(const gft_poly* a);                                   /* Neg                    mt:902-909 */
gft_poly* gft_mul(const gft_poly* a, const gft_poly* b);                /* Mul + mul/mul_1d       mt:971-1072 */
gft_poly* gft_div(const gft_poly* a, const gft_poly* b);                /* Div + div              mt:1162-1231 */
gft_poly* gft_exp(const gft_poly* a);                                   /* exp                    mt:406-417,1270-1317 */
gft_poly* gft_log(const gft_poly* a);                                   /* log                    mt:419-430,1319-1386 */
gft_poly* gft_pow(const gft_poly* a, uint32_t e);                       /* pow                    mt:433-451 */

/* ---- structure ---------------------------------------------------------------------------- */
gft_poly* gft_derivative(const gft_poly* a, size_t v, size_t n);        /* derivative             mt:457-481 */
gft_poly* gft_taylor_expansion_of_coeff(const gft_poly* a, size_t v, size_t n); /*                mt:484-509 */
gft_poly* gft_shift_down(const gft_poly* a, size_t v, size_t n);        /* shift_down (axis sum)  mt:514-536 */
/* Fused form of three reference calls: (derivative(a, v, 1).truncate_to_degree_p1(d) * var(v, x, d))
 * * from(c) — one step of the compound-Poisson observation loop, generating_function.rs:684-689 — same
 * per-element operation order, one kernel launch, no dispatch read-backs. */
gft_poly* gft_observe_step(const gft_poly* a, size_t v, const double* x, const double* c, size_t degree_p1);
/* n such steps in one call, innermost first: a <- gft_observe_step(a, v, x, cs + i*WIDTH, degree_p1 + (n - 1 - i)) for
 * i = 0..n-1 — the whole loop of generating_function.rs:684-689 as the evaluator unfolds it (each level one degree
 * lower than the one inside it).  One launch for the chain: every line along v runs all steps on its own. */
gft_poly* gft_observe_chain(const gft_poly* a, size_t v, const double* x, const double* cs, size_t n, size_t degree_p1);
/* The same for observations from a Poisson with a CONTINUOUS rate (generating_function.rs:703-706):
 * derivative(a, v, 1).truncate_to_degree_p1(d) * from(c), i.e. c * (x * ff) per element, in one launch. */
gft_poly* gft_derive_scale(const gft_poly* a, size_t v, const double* c, size_t degree_p1);
/* Fused form of derivative(a, v, n).truncate_to_degree_p1(degree_p1) — the evaluator's Derivative arm
 * (generating_function.rs:628-633: operand evaluated to degree_p1 + n, differentiated, cut back): one launch,
 * same values (truncation is slicing). */
gft_poly* gft_derivative_truncated(const gft_poly* a, size_t v, size_t n, size_t degree_p1);
gft_poly* gft_subst_var(const gft_poly* a, size_t v, const gft_poly* subst); /* subst_var (Taylor shift / marginalize / Horner) mt:540-580 */
gft_poly* gft_coefficients_of_term(const gft_poly* a, size_t v, size_t order); /*                 mt:341-358 */
gft_poly* gft_taylor_polynomial_terms(const gft_poly* a, size_t v, const size_t* orders,
                                      size_t n);                        /*                        mt:380-404 */
gft_poly* gft_truncate_to_degree_p1(const gft_poly* a, size_t degree_p1); /*                      mt:183-193 */
gft_poly* gft_remove_last_variable(const gft_poly* a);                  /*                        mt:172-181 */
gft_poly* gft_extend_to_dim(const gft_poly* a, size_t ndim, size_t degree_p1); /* extend          mt:81-89   */
gft_poly* gft_extend(const gft_poly* a, const size_t* new_size, size_t n); /* (test-only) extend  mt:91-112  */
/* (test-only) What the library currently claims, without looking at data, about where this handle's tensor holds coefficients
 * that are exactly [0,0]: kind 0 unknown, 1 measured irregular, 2 none, 3 exactly the leading slabs k_u < z[u],
 * 4 everything outside the box z[u] <= k_u < h[u], 5 all; z[8] and h[8] per axis (h is 0xffffffff where unbounded), and the
 * buffer's memoised linearity verdict (0 unknown, 1 not linear, 2 linear; 0 for a handle without a buffer).  Launches nothing,
 * reads nothing back and changes nothing a program can observe (the one thing it may fill is a host-side memo of whether a
 * scaling table holds a zero or a non-finite power).  gft_ (F64) has no such claims: kind 0.  Returns 0, or -1 with
 * gft_last_error() set if the library is not initialised. */
int gft_support_claim(const gft_poly* p, size_t* kind, size_t* z, size_t* h, size_t* lin_state);
gft_poly* gft_mul_var(const gft_poly* a, const double* m, size_t v, const size_t* shape,
                      const size_t* degrees_p1, size_t n);              /* mul_var                mt:589-608 */
gft_poly* gft_mul_linear(const gft_poly* a, const double* c, const double* m, size_t v,
                         const size_t* shape, const size_t* degrees_p1, size_t n); /* mul_linear  mt:611-623 */

/* ---- Interval<F64> twins (src/interval.rs; `--bounds`, main.rs:115-127) -------------------- */
/* Same functions with prefix gfti_; scalars are {lo,hi}, data is two planes (lo then hi).      */
#define GFT_DECLARE_INTERVAL_TWINS 1
const char* gfti_last_error(void);
int gfti_width(void);
gft_poly* gfti_from_host(const double* planes, const size_t* shape, const size_t* degrees_p1, size_t ndim);
gft_poly* gfti_from_device(const double* src, const int64_t* strides, const size_t* shape, const size_t* degrees_p1,
                           size_t ndim, void* stream);
gft_poly* gfti_scalar(const double* x);
gft_poly* gfti_from_u32(uint32_t c);
gft_poly* gfti_zero_with(const size_t* degrees_p1, size_t ndim);
gft_poly* gfti_var(size_t v, const double* x, size_t len);
gft_poly* gfti_var_at_zero(size_t v, size_t len);
gft_poly* gfti_var_with_degrees_p1(size_t v, const double* x, const size_t* degrees_p1, size_t ndim);
gft_poly* gfti_clone(const gft_poly* p);
void gfti_free(gft_poly* p);
size_t gfti_num_vars(const gft_poly* p);
size_t gfti_numel(const gft_poly* p);
void gfti_shape(const gft_poly* p, size_t* out);
void gfti_degrees_p1(const gft_poly* p, size_t* out);
int gfti_to_host(const gft_poly* p, double* out);
int gfti_to_device(const gft_poly* p, double* dst, const int64_t* strides, void* stream);
/* Batched series over Interval<F64>: gft_series_* on tensors [2, B..., n] = (lo, hi).  The argument lists are those of
 * gft_series_*, but every stride array (xbs / ybs / sbs / rbs) has nbatch + 1 entries: the FIRST is the lo -> hi plane stride in
 * elements (gfti_from_device's convention), the batch strides follow.  NULL = C-contiguous rows with the two planes back to
 * back.  The plane stride of an operand or of the seeds may be 0 (a point interval: x.expand(2, ...)); the result's must
 * separate its planes (the planes count as one more axis of "the rows do not overlap"), the overlap test covers both planes
 * of every operand, and "the same view" of an in-place result includes the plane stride.  Seeds are [2, B...].  n <= 2048:
 * with two planes the LDS footprints of gft_series_* at 4096 are reached there.  Per item the results are the reference's
 * general algorithms over Interval<F64> (interval.rs), each bound with the oracle's bits; gft_series_last_form and the
 * "series_form" option serve both families. */
int gfti_series_mul(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_div(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_exp(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_log(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_compose(const double* f, const int64_t* fbs, size_t nf, const double* g, const int64_t* gbs, size_t ng,
                        double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_pow(const double* x, const int64_t* xbs, size_t nx, uint32_t e, double* res, const int64_t* rbs, size_t n,
                    const size_t* batch, size_t nbatch, void* stream);
/* Batched series over BigFloat (big_float.rs): gft_series_mul / div / exp / log / compose / pow on tensors [2, B..., n] =
 * (factor, exponent).  These six are the whole BigFloat surface of the library: there is no handle family, no other rank and no
 * observation op.  The argument lists are those of gfti_series_*: every stride array (xbs / ybs / sbs / rbs) has nbatch + 1
 * entries, the FIRST the factor -> exponent plane stride in elements, the batch strides behind it; NULL = C-contiguous rows with
 * the two planes back to back.  No plane stride may be 0 (a factor plane cannot be its own exponent plane): refused on every operand,
 * on the seeds and on the result.  Everything else is judged as for gfti_series_*: the overlap test covers both planes, the result may
 * be an operand only as the same view (plane stride included), n <= 2048.  Seeds are [2, B...]; NULL: formed on the device
 * (exp2 / log2 of the device library: a few ulps from a host libm's, so exact bits need the caller's seeds).
 * The element contract: a coefficient is factor * 2^exponent; the factor is in +-[1, 2), or 0 with exponent 0, or non-finite (its
 * exponent is kept); the exponent is an integral double with |e| < 2^52; exponent differences of 2^31 or more are unsupported (the
 * reference truncates them to 32 bits).  Inputs are not scanned: values outside the contract give unspecified values, never an
 * out-of-bounds access.  Per item the results are the reference's general algorithms in BigFloat arithmetic, every factor and
 * exponent with the oracle's bits -- including every addition of zero the reference performs: 0 + b drops b at exponent <= -1024,
 * so mul adds each finished sum onto a zero (mul_rec onto its zeroed result), as do the products inside compose and pow.
 * gft_series_last_form and the "series_form" option serve this family too. */
int gftb_series_mul(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gftb_series_div(const double* x, const int64_t* xbs, size_t nx, const double* y, const int64_t* ybs, size_t ny,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gftb_series_exp(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gftb_series_log(const double* x, const int64_t* xbs, size_t nx, const double* seed, const int64_t* sbs,
                    double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gftb_series_compose(const double* f, const int64_t* fbs, size_t nf, const double* g, const int64_t* gbs, size_t ng,
                        double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gftb_series_pow(const double* x, const int64_t* xbs, size_t nx, uint32_t e, double* res, const int64_t* rbs, size_t n,
                    const size_t* batch, size_t nbatch, void* stream);
/* Batched bivariate series over Interval<F64>: gft_series2_* on tensors [2, B..., n0, n1] = (lo, hi).  The argument lists are those
 * of gft_series2_* (row strides `xrs` / `yrs` / `rrs` included, one per operand: both planes share it); the stride-array convention
 * is gfti_series_*'s: every batch-stride array (xbs / ybs / sbs / rbs) has nbatch + 1 entries, the lo -> hi plane stride FIRST, NULL =
 * C-contiguous items with the two planes back to back.  An operand's or the seeds' plane stride may be 0 (a point interval read
 * twice); the result's planes are distinct memory, the planes and the rows both join the proof that the result's elements are
 * distinct addresses, and "the same view" of an in-place result includes the plane stride.  Seeds are [2, B...]; NULL: formed on the
 * device by the interval exp / log of coefficient [0, 0].  n0 * n1 <= 2048: an interval occupies 16 bytes of LDS, so the footprints of
 * gft_series2_* at 4096 are reached there.  Per item the results are the loops stated above for gft_series2_mul / div / exp / log /
 * compose / pow with every step one operation of Interval<F64> (interval.rs: round to nearest, one ulp outwards, with its
 * short-circuits): sums start from [0,0] (and [0,0] + b is b), j and k enter as the point intervals from_u32(j), from_u32(k),
 * pow starts from [[[1,1]]].  Each bound carries the oracle's bits under the same rule as for gft_series2_*.  One workgroup per item;
 * gft_series_last_form() reports 2 afterwards. */
int gfti_series2_mul(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs,
                     int64_t yrs, size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1,
                     const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_div(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* y, const int64_t* ybs,
                     int64_t yrs, size_t ny0, size_t ny1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1,
                     const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_exp(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs,
                     double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                     void* stream);
int gfti_series2_log(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, const double* seed, const int64_t* sbs,
                     double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch,
                     void* stream);
int gfti_series2_compose(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, const double* g, const int64_t* gbs,
                         int64_t grs, size_t ng0, size_t ng1, int var, double* res, const int64_t* rbs, int64_t rrs, size_t n0,
                         size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_pow(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, uint32_t e, double* res,
                     const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);
/* Batched trivariate series over Interval<F64>: gft_series3_* on tensors [2, B..., n0, n1, n2] = (lo, hi).  The argument lists are those
 * of gft_series3_* (slab strides `xss` / `yss` / `rss` and row strides `xrs` / `yrs` / `rrs` included, one each per operand: both
 * planes share them); the stride-array convention is gfti_series_*'s: every batch-stride array (xbs / ybs / sbs / rbs) has nbatch + 1
 * entries, the lo -> hi plane stride FIRST, NULL = C-contiguous items with the two planes back to back.  An operand's or the seeds'
 * plane stride may be 0 (a point interval read twice); the result's planes are distinct memory, the planes, the slabs and the rows all
 * join the proof that the result's elements are distinct addresses, and "the same view" of an in-place result includes the plane
 * stride.  Seeds are [2, B...]; NULL: formed on the device by the interval exp / log of coefficient [0, 0, 0].  n0 * n1 * n2 <= 2048: an
 * interval occupies 16 bytes of LDS, so the footprints of gft_series3_* at 4096 are reached there.  Per item the results are the loops
 * stated above for gft_series3_mul / div / exp / log / compose / pow -- BOTH rules first: the stored result shape S decided by the
 * shapes alone, its unit axes squeezed, everything outside S [+0.0, +0.0] -- with every step one operation of Interval<F64>
 * (interval.rs: round to nearest, one ulp outwards, with its short-circuits):
 *   mul  z[k0][k1] = [0,0];  for j0, j1 ascending:  o = [0,0];  for j2 ascending: o = o + x[j0][j1][j2] * y[k0-j0][k1-j1][k2-j2];
 *        z[k0][k1][k2] = z[k0][k1][k2] + o       (the row sum from [0,0] first, then added; [0,0] + b is b)
 *   div  c = the sum over j0 in max(0, k0+1-ny0) .. k0-1 of r[j0] (*) y[k0-j0];  c = -c;  c[:nx1][:nx2] += x[k0];  r[k0] = div2(c, y[0])
 *   exp  r[0] = exp2(x[0], seed);  c = the sum over j0 in 1 .. min(nx0, k0+1)-1 of (x[j0] * from_u32(j0)) (*) r[k0-j0];
 *        r[k0] = c / from_u32(k0)
 *   log  r[0] = log2(x[0], seed);  c = the sum over j0 in max(1, k0+1-nx0) .. k0-1 of x[k0-j0] (*) (r[j0] * from_u32(j0));  c = -c;
 *        c[:nx1][:nx2] += from_u32(k0) * x[k0];  c = div2(c, x[0]);  r[k0] = c / from_u32(k0)
 * with (*) the slab product above and div2 / exp2 / log2 the loops of gfti_series2_div / exp / log; compose and pow are the chains of
 * gft_series3_compose / pow over that mul at the compact shapes, pow from [[[[1,1]]]].  Each bound carries the oracle's bits under the
 * same rule as for gft_series3_*, NaN for NaN.  pow's workspace is 2 * (3 * items * n0 * n1 * n2 + 1) doubles, plane-major, and the
 * plane axis joins its one copy of the operand: a batch with more than 9 non-contiguous axes is refused.  One workgroup per item;
 * where the runtime grants less LDS than an item needs the call fails and says so.  gft_series_last_form() reports 2 afterwards. */
int gfti_series3_mul(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* y,
                     const int64_t* ybs, int64_t yss, int64_t yrs, size_t ny0, size_t ny1, size_t ny2, double* res, const int64_t* rbs,
                     int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch, void* stream);
int gfti_series3_div(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* y,
                     const int64_t* ybs, int64_t yss, int64_t yrs, size_t ny0, size_t ny1, size_t ny2, double* res, const int64_t* rbs,
                     int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch, void* stream);
int gfti_series3_exp(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* seed,
                     const int64_t* sbs, double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2,
                     const size_t* batch, size_t nbatch, void* stream);
int gfti_series3_log(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, const double* seed,
                     const int64_t* sbs, double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2,
                     const size_t* batch, size_t nbatch, void* stream);
int gfti_series3_compose(const double* f, const int64_t* fbs, int64_t fss, int64_t frs, size_t nf0, size_t nf1, size_t nf2, const double* g,
                         const int64_t* gbs, int64_t gss, int64_t grs, size_t ng0, size_t ng1, size_t ng2, int var, double* res,
                         const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch, size_t nbatch,
                         void* stream);
int gfti_series3_pow(const double* x, const int64_t* xbs, int64_t xss, int64_t xrs, size_t nx0, size_t nx1, size_t nx2, uint32_t e,
                     double* res, const int64_t* rbs, int64_t rss, int64_t rrs, size_t n0, size_t n1, size_t n2, const size_t* batch,
                     size_t nbatch, void* stream);
/* The observation ops over Interval<F64>: gft_series_* / gft_series2_* derivative / taylor_expansion_of_coeff / shift_down /
 * evaluate_all_one on (lo, hi) planes, the stride-array convention of gfti_series_* (the plane stride first; 0 on the operand: point
 * intervals).  The same loops with every step one operation of the reference's interval arithmetic, its short-circuits included
 * ([0,0] + b is b: the sums start from [0,0], so the first addition changes nothing).  evaluate_all_one's result is [2, B...].  The
 * limits on the operand are nx <= 2048 and nx0 * nx1 <= 2048. */
int gfti_series_derivative(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,
                           const size_t* batch, size_t nbatch, void* stream);
int gfti_series_taylor_expansion_of_coeff(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs,
                                          size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_shift_down(const double* x, const int64_t* xbs, size_t nx, size_t k, double* res, const int64_t* rbs, size_t n,
                           const size_t* batch, size_t nbatch, void* stream);
int gfti_series_evaluate_all_one(const double* x, const int64_t* xbs, size_t nx, double* res, const int64_t* rbs, const size_t* batch,
                                 size_t nbatch, void* stream);
int gfti_series2_derivative(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,
                            const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_taylor_expansion_of_coeff(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k,
                                           double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,
                                           size_t nbatch, void* stream);
int gfti_series2_shift_down(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, int var, size_t k, double* res,
                            const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_evaluate_all_one(const double* x, const int64_t* xbs, int64_t xrs, size_t nx0, size_t nx1, double* res,
                                  const int64_t* rbs, const size_t* batch, size_t nbatch, void* stream);
/* The observation chains over Interval<F64>: gft_series_observe_chain / gft_series2_observe_chain on (lo, hi) planes, the plane
 * stride first in every stride array; x is [2, B...] and cs [2, B..., nsteps].  The same loops, every * and + the reference's Interval
 * operation with its own short-circuits ([0,0] + A is A; [0,0] * finite is [+0,+0]); a scalar equals 0 or 1 when both of its bounds
 * do.  The limits on the operand are na <= 2048 and na0 * na1 <= 2048. */
int gfti_series_observe_chain(const double* a, const int64_t* abs, size_t na, const double* x, const int64_t* xbs, const double* cs,
                              const int64_t* cbs, size_t nsteps, size_t degree_p1, double* res, const int64_t* rbs, size_t n,
                              const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_observe_chain(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* x,
                               const int64_t* xbs, const double* cs, const int64_t* cbs, size_t nsteps, size_t degree_p1, double* res,
                               const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch, size_t nbatch, void* stream);
/* The negative-binomial observation over Interval<F64>: the three calls above on (lo, hi) planes, the plane stride first in every
 * stride array; p and x are [2, B...], ls and the Lah row [2, B..., K + 1].  The same loops in the reference's Interval operations.
 * The limits: order + 1 <= 2048; na <= 2048, na0 * na1 <= 2048 and 3 * degree_p1 + K <= 4096. */
int gfti_series_lah_row(const double* p, const int64_t* pbs, size_t order, double* res, const int64_t* rbs, const size_t* batch, size_t nbatch,
                        void* stream);
int gfti_series_observe_negbinomial(const double* a, const int64_t* abs, size_t na, const double* x, const int64_t* xbs, const double* p,
                                    const int64_t* pbs, const double* ls, const int64_t* lbs, size_t nls, size_t degree_p1, double* res,
                                    const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_observe_negbinomial(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* x,
                                     const int64_t* xbs, const double* p, const int64_t* pbs, const double* ls, const int64_t* lbs, size_t nls,
                                     size_t degree_p1, double* res, const int64_t* rbs, int64_t rrs, size_t n0, size_t n1, const size_t* batch,
                                     size_t nbatch, void* stream);
/* The affine substitutions over Interval<F64>: gft_series_mul_linear / gft_series_compose_linear and their rank-2 twins on (lo, hi)
 * planes, the plane stride first in every stride array; c and m are [2, B...].  The same loops, every * and + the reference's Interval
 * operation with its own short-circuits; c equals 0 when both of its bounds do.  The limits on the result are n <= 2048 and
 * n0 * n1 <= 2048. */
int gfti_series_mul_linear(const double* a, const int64_t* abs, size_t na, const double* c, const int64_t* cbs, const double* m,
                           const int64_t* mbs, double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_mul_linear(const double* a, const int64_t* abs, int64_t ars, size_t na0, size_t na1, int var, const double* c,
                            const int64_t* cbs, const double* m, const int64_t* mbs, double* res, const int64_t* rbs, int64_t rrs, size_t n0,
                            size_t n1, const size_t* batch, size_t nbatch, void* stream);
int gfti_series_compose_linear(const double* f, const int64_t* fbs, size_t nf, const double* c, const int64_t* cbs, const double* m,
                               const int64_t* mbs, double* res, const int64_t* rbs, size_t n, const size_t* batch, size_t nbatch, void* stream);
int gfti_series2_compose_linear(const double* f, const int64_t* fbs, int64_t frs, size_t nf0, size_t nf1, int var, int wvar, const double* c,
                                const int64_t* cbs, const double* m, const int64_t* mbs, double* res, const int64_t* rbs, int64_t rrs, size_t n0,
                                size_t n1, const size_t* batch, size_t nbatch, void* stream);
size_t gfti_len_of(const gft_poly* p, size_t v);
int gfti_is_constant(const gft_poly* p);
int gfti_is_zero(const gft_poly* p);
int gfti_is_one(const gft_poly* p);
int gfti_equal(const gft_poly* a, const gft_poly* b);
long gfti_format(const gft_poly* p, int debug, char* out, size_t cap);
int gfti_constant_term(const gft_poly* p, double* out);
int gfti_extract_constant(const gft_poly* p, double* out);
int gfti_extract_linear(const gft_poly* p, double* c, double* m, size_t* v);
int gfti_coefficient(const gft_poly* p, const size_t* index, size_t n, double* out);
gft_poly* gfti_add(const gft_poly* a, const gft_poly* b);
gft_poly* gfti_sub(const gft_poly* a, const gft_poly* b);
gft_poly* gfti_add_scaled(const gft_poly* a, const gft_poly* b, const double* c);
gft_poly* gfti_neg(const gft_poly* a);
gft_poly* gfti_mul(const gft_poly* a, const gft_poly* b);
gft_poly* gfti_div(const gft_poly* a, const gft_poly* b);
gft_poly* gfti_exp(const gft_poly* a);
gft_poly* gfti_log(const gft_poly* a);
gft_poly* gfti_pow(const gft_poly* a, uint32_t e);
gft_poly* gfti_derivative(const gft_poly* a, size_t v, size_t n);
gft_poly* gfti_taylor_expansion_of_coeff(const gft_poly* a, size_t v, size_t n);
gft_poly* gfti_shift_down(const gft_poly* a, size_t v, size_t n);
gft_poly* gfti_observe_step(const gft_poly* a, size_t v, const double* x, const double* c, size_t degree_p1);
gft_poly* gfti_observe_chain(const gft_poly* a, size_t v, const double* x, const double* cs, size_t n, size_t degree_p1);
gft_poly* gfti_derive_scale(const gft_poly* a, size_t v, const double* c, size_t degree_p1);
gft_poly* gfti_derivative_truncated(const gft_poly* a, size_t v, size_t n, size_t degree_p1);
gft_poly* gfti_subst_var(const gft_poly* a, size_t v, const gft_poly* subst);
gft_poly* gfti_coefficients_of_term(const gft_poly* a, size_t v, size_t order);
gft_poly* gfti_taylor_polynomial_terms(const gft_poly* a, size_t v, const size_t* orders, size_t n);
gft_poly* gfti_truncate_to_degree_p1(const gft_poly* a, size_t degree_p1);
gft_poly* gfti_remove_last_variable(const gft_poly* a);
gft_poly* gfti_extend_to_dim(const gft_poly* a, size_t ndim, size_t degree_p1);
gft_poly* gfti_extend(const gft_poly* a, const size_t* new_size, size_t n);
int gfti_support_claim(const gft_poly* p, size_t* kind, size_t* z, size_t* h, size_t* lin_state);
gft_poly* gfti_mul_var(const gft_poly* a, const double* m, size_t v, const size_t* shape,
                       const size_t* degrees_p1, size_t n);
gft_poly* gfti_mul_linear(const gft_poly* a, const double* c, const double* m, size_t v, const size_t* shape,
                          const size_t* degrees_p1, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* GFTAYLOR_H */

/*
 * tsim_hip.h - C ABI of the MI355X (gfx950) stabilizer-rank sampling engine.
 *
 * This is the drop-in boundary for the one hot path of QuEraComputing/tsim:
 *
 *     tsim.sampler.sample_program(program, f_params, key) -> bool[B, num_outputs]
 *                                       (reference: src/tsim/sampler.py:117-167)
 *     tsim.compile.evaluate.evaluate(circuit, param_vals) -> complex64[B]
 *                                       (reference: src/tsim/compile/evaluate.py:15-59)
 *
 * The reference is pure Python/JAX and has no FFI of its own; these entry
 * points are what a binding for that seam binds (the ctypes stub is shown in
 * INTEGRATION.md, the shipped one is tsim_amd/_lib.py).  Plain pointers and
 * sizes only - no torch / numpy / jax types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative TSIM_E* code and never
 *     throws or prints; tsim_last_error() returns a thread-local message;
 *   - "program description" arrays use EXACTLY the reference layout: one byte
 *     per bit, row-major, padded to the per-family maximum term count
 *     (src/tsim/compile/compile.py:21-37, src/tsim/compile/terms.py:42-207);
 *     the library bit-packs them and uploads them once per device;
 *   - a handle is bound to one HIP device; calls on one handle must not race;
 *   - packed shot rows are little-endian bit strings: bit i of a row lives in
 *     64-bit word i/64 at position i%64 (== numpy.packbits(bitorder="little")).
 */
#ifndef TSIM_HIP_H
#define TSIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSIM_OK 0
#define TSIM_EINVAL (-22)      /* bad argument / malformed program           */
#define TSIM_ENOMEM (-12)      /* host or device allocation failed            */
#define TSIM_EHIP (-5)         /* a HIP runtime call failed                   */
#define TSIM_ENOTSUP (-95)     /* program exceeds a compiled-in limit         */
#define TSIM_ESTATE (-1)       /* call not valid in the handle's state        */

#define TSIM_MAX_PARAMS 2048   /* max n_params (f bits + outputs) per level   */

typedef struct tsim_program tsim_program;

/*
 * One autoregressive level == one reference CompiledScalarGraphs
 * (src/tsim/compile/compile.py:21-37).  G = num_graphs, P = n_params.
 */
typedef struct tsim_level_desc {
  int32_t num_graphs;            /* G */
  int32_t n_params;              /* P */
  int32_t ta, tb, tc, td;        /* padded term counts of the four families   */
  /* NodePhases   (terms.py:42-73)   */
  const uint8_t *a_phases;       /* [G, ta]     values 0..7                   */
  const uint8_t *a_params;       /* [G, ta, P]  0/1                           */
  const int32_t *a_counts;       /* [G]         real terms per graph          */
  /* HalfPiPhases (terms.py:76-107)  */
  const uint8_t *b_coeffs;       /* [G, tb]     0,2,4,6 (0 = padding)         */
  const uint8_t *b_params;       /* [G, tb, P]                                */
  /* PiProducts   (terms.py:110-144) */
  const uint8_t *c_psi_const;    /* [G, tc]                                   */
  const uint8_t *c_psi_params;   /* [G, tc, P]                                */
  const uint8_t *c_phi_const;    /* [G, tc]                                   */
  const uint8_t *c_phi_params;   /* [G, tc, P]                                */
  /* PhasePairs   (terms.py:147-187) */
  const uint8_t *d_alpha;        /* [G, td]     values 0..7                   */
  const uint8_t *d_alpha_params; /* [G, td, P]                                */
  const uint8_t *d_beta;         /* [G, td]                                   */
  const uint8_t *d_beta_params;  /* [G, td, P]                                */
  const int32_t *d_counts;       /* [G]                                       */
  /* ScalarPrefactor (terms.py:190-207) */
  const uint8_t *phase_indices;  /* [G]   0..7                                */
  const int32_t *floatfactor;    /* [G,4] (a,b,c,d) on basis (1,w,i,conj w)   */
  const int32_t *power2;         /* [G]                                       */
  const float *approx;           /* [G,2] complex64 (re,im); may be NULL      */
  int32_t has_approx;            /* static flag has_approximate_floatfactors  */
} tsim_level_desc;

/* ---- program construction (replaces the device upload implied by
 *      jnp.asarray of a CompiledProgram, src/tsim/core/types.py:80-107) ---- */

/* direct_f_indices/direct_flips: [n_direct]; output_order: [num_outputs]
 * (direct entries first, then the compiled components in processing order). */
int tsim_program_create(int32_t num_outputs, int32_t num_detectors, int32_t n_direct,
                        const int32_t *direct_f_indices, const uint8_t *direct_flips,
                        const int32_t *output_order, tsim_program **out);

/* Adds a CompiledComponent (types.py:55-77); components must be added in the
 * reference's processing order.  n_levels is n_out+1 (sequential mode) or 2
 * (joint mode, evaluate-only).  Returns the component index (>= 0). */
int tsim_program_add_component(tsim_program *p, int32_t n_out, const int32_t *output_indices,
                               int32_t F, const int32_t *f_selection, int32_t n_levels);

/* Adds the next level of component `component` (arrays are copied/packed). */
int tsim_program_add_level(tsim_program *p, int32_t component, const tsim_level_desc *level);

/*
 * Evaluation formulation, to be set before finalize (default TSIM_MODE_AUTO; the environment
 * variable TSIM_AMD_MODE=faithful forces TSIM_MODE_FAITHFUL):
 *   TSIM_MODE_FAITHFUL  operation-by-operation mirror of the reference's int32 arithmetic
 *                       (src/tsim/core/exact_scalar.py:19-137), identical even where it wraps;
 *   TSIM_MODE_AUTO      use the faster exact-value formulation (NodePhases by class counting,
 *                       phase exponent as a Dickson-reduced GF(2) quadratic form, pack-time term
 *                       tables; LDS chunk-table kernel when every component has <= 64 parameters - since
 *                       round 5 up to 80 with <= 64 selected f bits, and up to 128 for components of many graphs)
 *                       whenever every graph qualifies (<= 30 NodePhases terms,
 *                       even HalfPi coefficients, small floatfactors); it yields the same canonical
 *                       (a,b,c,d,power) and float32 amplitude as the reference whenever the
 *                       reference's own int32 arithmetic does not wrap.
 */
#define TSIM_MODE_AUTO 0
#define TSIM_MODE_FAITHFUL 1
#define TSIM_MODE_ROW_KERNEL 2   /* exact-value formulation, but the row-by-row kernel instead of the
                                    LDS chunk-table kernel (k_sample4); for tests and A/B timing */
int tsim_program_set_mode(tsim_program *p, int32_t mode);
/* after finalize: *fast = 1 if the exact-value formulation was selected */
int tsim_program_get_mode(const tsim_program *p, int32_t *fast);

/*
 * Low-weight error-pattern tables (before finalize).  The Bernoulli thresholds p1/prev of
 * _sample_component (sampler.py:54-79) depend on a shot only through the component's selected
 * f bits and the outcome prefix; for f_sel patterns of weight <= max_weight (0..7, as many as fit a
 * 1 GiB table per component; TSIM_AMD_PATTERN_TABLE_MB overrides) they are tabulated by the sampling kernels' own
 * arithmetic, and shots carrying such patterns in every component are finished by a light first
 * pass (one Threefry draw + one table read per output); only the remaining rows run the full
 * kernel.  Bit-identical results.  Requires <= 12 outputs and <= 64 parameters per component (round 5: <= 128, see
 * TSIM_MODE_AUTO above) - or, for the programs of the sparse-column kernels (any number of components of up to 511
 * selected f bits in ascending order, <= 8 outputs each, f indices below 2048): weight <= 4, below 4 GiB per component
 * (C(200, <= 4) patterns of 8 thresholds are 2.1 GB), built on the device by unranking the pattern index.
 *   enable: 1 on, 0 off, -1 default (on in TSIM_MODE_AUTO);  max_weight: 0..7 pins the depth and builds it at finalize;
 *   -1 (round 5) = the deepest tables that cost about half a millisecond at finalize (weight 3-4), the default depth -
 *   5, or 4 for the sparse-column programs - built in the background and put in place at a later launch
 *   (tsim_program_tables_pending), one more weight (up to 7) after ~10^10 rows that leave too many rows to the
 *   full kernels (TSIM_AMD_DEEP_TABLES=1: at once; -1: never).
 * The environment variable TSIM_AMD_PATTERN_TABLES=0/1 overrides `enable`.
 * Launch plan: the hard-row kernel reports the number of hard rows of each launch through mapped
 * host memory; when most rows of recent launches were hard (dense error patterns) the following
 * launches skip the first pass (re-probing every 16th launch), and when the hard-row lists are
 * short the overflow launch of the full kernel is dropped.  TSIM_AMD_ADAPTIVE=0 pins the default
 * plan.  Results never depend on the plan.
 */
int tsim_program_set_pattern_tables(tsim_program *p, int32_t enable, int32_t max_weight);
/* after finalize: *enabled, table bytes, and max tabulated weight per component ([n_components],
 * may be NULL) */
int tsim_program_pattern_table_info(const tsim_program *p, int32_t *enabled, int64_t *table_bytes,
                                    int32_t *max_weight);
/* *pending = 1 while pattern tables of another depth are being built in the background (the shallow start's default
 * depth, or a deeper one the launch plan asked for); they are put in place at a later launch.  Rates measured while
 * this is 1 are those of the transient.  (No reference counterpart: tsim_amd's own table machinery.) */
int tsim_program_tables_pending(const tsim_program *p, int32_t *pending);

/* Packs all levels into the device image and uploads it to HIP device `device`. */
int tsim_program_finalize(tsim_program *p, int32_t device);

void tsim_program_destroy(tsim_program *p);

/* ---- the hot path ---------------------------------------------------- */

/*
 * sample_program for one batch, host buffers in the reference layout
 * (replaces src/tsim/sampler.py:117-167 incl. the H2D at :398 and D2H at :415).
 *   f            uint8 [B, num_f], nonzero == 1
 *   key_hi/lo    the post-split Threefry-2x32 subkey handed to sample_program
 *                (src/tsim/sampler.py:399)
 *   shot_offset  in-batch index of row 0 (Threefry counter of shot s is
 *                shot_offset+s): a batch sharded over devices reproduces the
 *                unsharded result bit for bit
 *   out          out_packed == 0: uint8 [B, num_outputs] (0/1)
 *                out_packed != 0: uint8 [B, 8*ceil(num_outputs/64)] little-endian bits
 *   max_norm_dev float [n_components] (may be NULL): max |norm-1| of the
 *                normalisation check of src/tsim/sampler.py:71-72, valid only
 *                when the call contains in-batch shot 0 (else left untouched)
 */
int tsim_sample_batch(tsim_program *p, const uint8_t *f, int64_t B, int32_t num_f,
                      uint32_t key_hi, uint32_t key_lo, int64_t shot_offset,
                      uint8_t *out, int32_t out_packed, float *max_norm_dev);

/*
 * Same, on device-resident packed buffers (no host transfer, asynchronous on
 * `stream`; pass NULL for the handle's own stream):
 *   d_f    uint64 [B, ceil(num_f/64)]   packed error-mechanism rows
 *   d_out  uint64 [B, ceil(num_outputs/64)]
 *   d_max_norm_dev  device float [n_components] or NULL
 */
int tsim_sample_batch_device(tsim_program *p, const uint64_t *d_f, int64_t B, int32_t num_f,
                             uint32_t key_hi, uint32_t key_lo, int64_t shot_offset,
                             uint64_t *d_out, float *d_max_norm_dev, void *stream);

/*
 * Pipelined form of tsim_sample_batch_device.  With the pattern tables active a launch is two
 * passes; the second one (a few thousand "hard" rows, latency-bound) does not need the GPU to
 * itself.  Each `slot` (0 .. TSIM_PIPELINE_SLOTS-1) owns a stream - a lane (slot 0's lane is the handle's
 * own stream, tsim_get_stream: it sits on a hardware queue of its own); _begin enqueues the whole
 * launch on the slot's lane, so launches of one slot are ordered among themselves and launches of
 * different slots overlap (the second pass of one under the first pass of the next).  The lane first
 * waits for the work already queued on `stream` (the producer of d_f) unless `flags` has
 * TSIM_PIPE_INPUTS_READY (inputs complete, and nothing queued on `stream` still uses d_out): then no
 * cross-stream event is needed at all.  _end makes `stream` wait for the slot's lane - only after
 * _end (and the usual stream ordering) are d_out / d_max_norm_dev complete.  The caller must not reuse
 * the buffers of a slot for anything else between _begin and _end.  Results are identical to the
 * serial call.  Keep the number of busy streams (lanes + the caller's + RCCL's) at 4 or fewer: beyond
 * the 4 hardware queues HIP uses, launches slow down by 3x on this stack.
 *
 * Deferred second pass.  When recent launches left few hard rows (the launch-plan feedback: longest
 * list <= 192), _begin only enqueues the FIRST pass, alternating between the lanes of slots 0 and 1,
 * and keeps the launch's hard rows for a batch: every TSIM_AMD_DEFER_GROUP (default 4; 8 for programs with
 * more than 4 MB of chunk tables, whose hard-row pass is long) launches - or
 * when _end / _begin / tsim_synchronize needs a slot whose rows are still waiting - ONE grid
 * (k_sample4h_multi) serves the hard rows of all waiting launches on the lane of slot 2, after their
 * first passes.  No lane then waits for a second pass before its next first pass; a slot's next
 * launch still waits for the batch that served its previous one (an event query, a stream wait only
 * if needed), so the number of SLOTS in flight - 8 is enough on C2 - hides the batch latency, not the
 * number of lanes.  The number of hard-row lists follows the load (4..64, about 40 rows each) so that
 * the 64-row blocks of the hard-row kernel are filled.  TSIM_AMD_DEFER_HARD=0 / TSIM_AMD_MERGE_LISTS=0
 * switch these off.  Results never depend on any of it.
 */
#define TSIM_PIPELINE_SLOTS 32
#define TSIM_PIPE_INPUTS_READY 1u
/* d_out receives the reference's bit_packed rows, uint8 [B, ceil(num_outputs/8)] (sampler.py:665-669), INSTEAD of
 * the padded 8-byte words: ceil(n/8) bytes written per shot (3 instead of 8 for 20 outputs); any alignment */
#define TSIM_PIPE_OUT_BIT_PACKED 2u
int tsim_sample_batch_device_begin(tsim_program *p, int32_t slot, const uint64_t *d_f, int64_t B,
                                   int32_t num_f, uint32_t key_hi, uint32_t key_lo, int64_t shot_offset,
                                   uint64_t *d_out, float *d_max_norm_dev, void *stream, uint32_t flags);
int tsim_sample_batch_device_end(tsim_program *p, int32_t slot, void *stream);
/* Non-consuming form of _end: `stream` (NULL: the handle's stream) waits for the launch `slot` carried LAST, whether or
 * not a stream has been joined to it before (_end marks the slot as joined and a second _end adds no wait).  What a
 * producer needs before it overwrites the slot's INPUT buffer - the reference has no such hazard, its batches are
 * synchronous (sampler.py:398-404) - when a consumer stream already took the slot's output. */
int tsim_pipeline_wait_slot(tsim_program *p, int32_t slot, void *stream);
/* Make every pipeline lane wait for the work already queued on `stream` (NULL: the handle's stream) -
 * one event for all lanes.  Launches whose buffers depend only on that work may then pass
 * TSIM_PIPE_INPUTS_READY (bench.py: once per gather group instead of once per launch). */
int tsim_pipeline_wait_stream(tsim_program *p, void *stream);
/* tsim_sample_batch_device_end(slot, stream) for every slot that has a launch in flight: `stream` is then behind everything the
 * pipeline has been given (one call; NULL = the handle's stream). */
int tsim_pipeline_join(tsim_program *p, void *stream);
/* The stream of lane `lane` (= of slot `lane`; created on demand).  Lane 2 is where the deferred
 * hard-row batches run, i.e. where results complete: a consumer that joins its slots on THAT stream
 * (tsim_sample_batch_device_end(p, slot, lane2)) and queues its own work there (bench.py: the RCCL
 * gather) never makes a first-pass lane wait. */
int tsim_pipeline_lane_stream(tsim_program *p, int32_t lane, void **stream);
/* The NEXT _begin on `slot` also writes its rows as uint8[B, ceil(num_outputs/8)] into d_compact (the
 * reference's bit_packed layout, sampler.py:665-669) straight from the sampling kernels - no separate
 * compaction kernel.  One-shot: cleared by that launch. */
int tsim_pipeline_set_compact_output(tsim_program *p, int32_t slot, uint8_t *d_compact);
/* The same for a run of launches: the next `count` pipelined launches (any slot, in call order) write
 * their bit_packed rows to d_base, d_base + stride_bytes, ... - one call per gather group instead of one
 * per launch.  A per-slot buffer set with tsim_pipeline_set_compact_output takes precedence. */
int tsim_pipeline_set_compact_series(tsim_program *p, uint8_t *d_base, int64_t stride_bytes, int32_t count);
/* Between _begin and _end of `slot`: tsim_compact_rows_device of the launch's output rows, enqueued
 * on the slot's lane behind the launch; _end then also covers d_out. */
int tsim_sample_batch_device_compact(tsim_program *p, int32_t slot, const uint64_t *d_rows, int64_t B,
                                     int32_t nbits, uint8_t *d_out, void *stream);

/*
 * Device-side post-selection (the shot-skipping of src/tsim/sampler.py:422-545, done in HBM):
 *   tsim_postselect_device writes every row's DIRECT output bits to d_out (compiled columns 0),
 *   tests ((row ^ ref) & mask) != 0 per row (mask/ref: packed uint64 [ceil(num_outputs/64)] in final
 *   column order; ref may be NULL) and appends the surviving row numbers to d_row_index
 *   (uint32 [B], unordered), their count to d_row_count; d_discarded (uint8 [B]) is optional.
 *   tsim_sample_rows_device then samples only the listed rows (overwriting their d_out rows with
 *   direct + compiled bits).  The Threefry counter of a row stays its own in-batch index, so the
 *   result does not depend on the order of the list.
 */
int tsim_postselect_device(tsim_program *p, const uint64_t *d_f, int64_t B, int32_t num_f,
                           const uint64_t *d_mask, const uint64_t *d_ref, uint64_t *d_out,
                           uint32_t *d_row_index, uint32_t *d_row_count, uint8_t *d_discarded, void *stream);
int tsim_sample_rows_device(tsim_program *p, const uint64_t *d_f, int64_t B, int32_t num_f,
                            uint32_t key_hi, uint32_t key_lo, int64_t shot_offset, uint64_t *d_out,
                            float *d_max_norm_dev, const uint32_t *d_row_index, const uint32_t *d_row_count,
                            void *stream);

/*
 * evaluate(circuit, param_vals) for level `level` of component `component`
 * (replaces src/tsim/compile/evaluate.py:15-59).
 *   params        uint8 [B, n_params]
 *   re, im        float [B]  complex64 amplitude
 *   abs_out       optional float [B]: |amplitude| as jnp.abs(complex64) forms it
 *                 (the marginal of src/tsim/sampler.py:54,67,945,951)
 *   coeffs_power  optional int32 [B,5]: exact (a,b,c,d,power) of the summed
 *                 amplitude on the exact branch (zeros on the approximate one)
 */
int tsim_evaluate(tsim_program *p, int32_t component, int32_t level, const uint8_t *params,
                  int64_t B, float *re, float *im, float *abs_out, int32_t *coeffs_power);

/* ---- device-side data-format kernels either side of the path ---------- */

/* uint8 [B,num_f] (device) -> packed uint64 [B,ceil(num_f/64)] (device)      */
int tsim_pack_bits_device(tsim_program *p, const uint8_t *d_in, int64_t B, int32_t nbits,
                          uint64_t *d_out, void *stream);
/* packed uint64 [B,ceil(nbits/64)] (device) -> uint8 [B,nbits] (device)      */
int tsim_unpack_bits_device(tsim_program *p, const uint64_t *d_in, int64_t B, int32_t nbits,
                            uint8_t *d_out, void *stream);
/* uint64[B, in_words] padded rows -> uint8[B, ceil(nbits/8)] rows holding the first nbits columns:
 * the reference's bit_packed=True layout (np.packbits(bits[:, :nbits], axis=1, bitorder="little"),
 * sampler.py:665-669) - what a gather or a packed D2H has to move (3 instead of 8 bytes per shot for
 * 20 outputs).  in_words = 0: ceil(nbits/64).  d_out 4-byte aligned. */
int tsim_compact_rows_device(tsim_program *p, const uint64_t *d_in, int64_t B, int32_t in_words,
                             int32_t nbits, uint8_t *d_out, void *stream);
/* Post-selection after sampling (sampler.py:422-545 for device-side noise, where no host stream decides which shots reach
 * sample_program): rows of `row_bytes` bytes each (padded words or bit_packed); d_masks = 5 x row_bytes bytes: test mask,
 * reference XORed before the test, columns a discarded row keeps, XOR for surviving rows, XOR for discarded rows;
 * d_gone (optional) receives 0/1 per row. */
int tsim_postselect_rows_device(tsim_program *p, uint8_t *d_rows, int64_t B, int32_t row_bytes, const uint8_t *d_masks,
                                uint8_t *d_gone, void *stream);
/* The survivors of a chunk (d_gone[i] == 0, from tsim_postselect_device), IN SHOT ORDER, appended to a device-resident
 * queue of shot ids: queue[*d_tail ...] = base + i, *d_tail += their number (the reference's compacted batches,
 * sampler.py:466-508: the order fixes the survivors' Threefry counters).  d_scratch: ceil(n / 1024) uint32. */
int tsim_survivors_append_device(tsim_program *p, const uint8_t *d_gone, int64_t n, uint32_t base, uint32_t *d_scratch,
                                 uint32_t *d_queue, uint32_t *d_tail, void *stream);
/* The epilogue of CompiledDetectorSampler.sample (sampler.py:850-868: detectors / observables prepended, appended,
 * separate; reference-sample flips) and _maybe_bit_pack (:665-669) on the device: out column c = in column
 * (d_cols[c] & 0x7FFFFFFF) XOR (d_cols[c] >> 31) of the padded rows, one byte per column (packed = 0) or
 * ceil(n_cols / 8) bytes per row (packed = 1, np.packbits little-endian). */
int tsim_arrange_rows_device(tsim_program *p, const uint64_t *d_in, int64_t B, int32_t in_words, const uint32_t *d_cols,
                             int32_t n_cols, int32_t packed, uint8_t *d_out, void *stream);

/* Row gather / scatter by index on packed rows of `words` 64-bit words - the data movement of the
 * reference's host-noise post-selection (src/tsim/sampler.py:466-508: survivors are compacted into dense
 * batches of batch_size, the last one padded with its first row; result rows go back to the shots they
 * came from):
 *   gather : d_dst[i] = d_src[d_index[i < n_valid ? i : 0]]   for i < n_total
 *   scatter: d_dst[d_index[i]] = d_src[i]                      for i < n                    */
int tsim_gather_rows_device(tsim_program *p, const uint64_t *d_src, int32_t words, const uint32_t *d_index,
                            int64_t n_valid, int64_t n_total, uint64_t *d_dst, void *stream);
int tsim_scatter_rows_device(tsim_program *p, const uint64_t *d_src, int32_t words, const uint32_t *d_index,
                             int64_t n, uint64_t *d_dst, void *stream);

/* ---- host-side noise sampler ON NUMPY'S STREAM (bit-exact replacement of ChannelSampler.sample,
 *      src/tsim/noise/channels.py:624-658, for a numpy Generator backed by PCG64; no device involved) --------- */

/* PCG64 state and increment as numpy's bit_generator.state reports them (128-bit integers, split in halves) */
typedef struct tsim_pcg64 {
  uint64_t state_lo, state_hi, inc_lo, inc_hi;
} tsim_pcg64;

#define TSIM_PCG_RAW 0          /* Generator.bit_generator.random_raw  -> uint64 */
#define TSIM_PCG_DOUBLE 1       /* Generator.random / uniform(0, 1)    -> double */
#define TSIM_PCG_EXPONENTIAL 2  /* Generator.standard_exponential      -> double (ziggurat) */
#define TSIM_PCG_GEOMETRIC 3    /* Generator.geometric(p)              -> int64  */
/* n draws of one kind; `rng` is advanced exactly as numpy advances it */
int tsim_pcg_draw(tsim_pcg64 *rng, int32_t kind, double p, int64_t n, void *out);

/* One ChannelSampler.sample(num_samples) call: per channel c (tables as _precompute_sparse builds them,
 * channels.py:578-622) n_draws = int(B p + 7 sqrt(B p (1 - p))) + 100 geometric gaps, positions = cumsum - 1
 * (those < B fire), one uniform per fired row, outcome = searchsorted(cond_cdf_c, u), row ^= pattern.
 *   n_outcomes[c]  non-identity outcomes of channel c;  cond_cdf  concatenated conditional CDFs;
 *   patterns       uint64 [sum n_outcomes, words] packed XOR patterns;  rows  uint64 [num_samples, words] (overwritten)
 *   threads        worker threads of the scatter pass (0: up to 8).  The stream consumption is sequential. */
int tsim_pcg_sample_channels(tsim_pcg64 *rng, int32_t n_channels, const double *p_fire, const int32_t *n_outcomes,
                             const double *cond_cdf, const uint64_t *patterns, int32_t words, int64_t num_samples,
                             uint64_t *rows, int32_t threads);

/* ---- device-side noise sampler (statistical replacement of ChannelSampler.sample,
 *      src/tsim/noise/channels.py:578-658; the numpy PCG64 stream is not reproduced) ---------- */
typedef struct tsim_noise tsim_noise;

/* Channel tables exactly as ChannelSampler._precompute_sparse builds them (channels.py:578-622):
 *   p_fire[n_channels]; n_outcomes[c] = number of non-identity outcomes of channel c;
 *   cond_cdf = the concatenated conditional CDFs; xor_patterns = uint8 [sum n_outcomes, num_f].
 * The sampler lives on the program's device and stream. */
int tsim_noise_create(tsim_program *p, int32_t num_f, int32_t n_channels, const double *p_fire,
                      const int32_t *n_outcomes, const double *cond_cdf, const uint8_t *xor_patterns,
                      tsim_noise **out);
/* d_f: uint64 [B, ceil(num_f/64)] (device); overwritten with a fresh batch keyed by (key_hi, key_lo). */
int tsim_noise_sample_device(tsim_noise *n, int64_t B, uint32_t key_hi, uint32_t key_lo, uint64_t *d_f,
                             void *stream);
/* What tsim_noise_create fixed, for tests and tuning:
 *   out[0] the kernel tsim_noise_sample_device launches: 0 k_noise_wave, 1 k_noise_tile, 2 k_noise (-1: no channels,
 *          the rows are only zeroed);
 *   out[1] wave_tile (shots per block of k_noise_wave, 0 when that form does not apply), out[2] wave_g (lanes per
 *          channel group), out[3] tile (shots per block of k_noise_tile, 0: rows too wide), out[4] tseg (its
 *          sub-segment), out[5] seg (shots per thread of k_noise);
 *   out[6] 1 when tsim_sample_steps_noise_device may fuse the noise into the first pass; out[7] words per f row. */
int tsim_noise_info(tsim_noise *n, int64_t out[8]);
/* tsim_sample_steps_device with the f rows drawn on the device, in the same call (the reference's batch loop,
 * src/tsim/sampler.py:393-400: channel sampler, then sample_program, per batch).  Batch j's noise key is the j-th
 * split of noise_key (advanced like `key`); its f rows are written to d_f[j] - the bytes tsim_noise_sample_device
 * writes for that key.  Programs of one component of at most 8 outputs over f rows of at most 128 bits draw the noise
 * INSIDE their first pass (one kernel: csrc/tsim_noise_fused.hip.h); every other program runs the noise kernel in
 * front of its first pass.  Results do not depend on which.  A call rejected before its first launch moves neither key. */
int tsim_sample_steps_noise_device(tsim_program *p, tsim_noise *n, int32_t n_steps, uint64_t *const *d_f, int64_t B,
                                   int32_t num_f, uint32_t key[2], uint32_t noise_key[2], int64_t shot_offset,
                                   void *const *d_out, float *const *d_max_norm_dev, uint32_t flags);
void tsim_noise_destroy(tsim_noise *n);

/* ---- measurements -> detection events (replaces Circuit.compile_m2d_converter, src/tsim/circuit.py:423-456, which
 *      hands the work to stim's CompiledMeasurementsToDetectionEventsConverter) --------------------------------------
 * Per shot, out_j = ref_j XOR (XOR of m_k over k in cols[row_ptr[j] .. row_ptr[j+1]-1]): a GF(2) affine map over the
 * measurement record.  A handle of its own, bound to HIP device `device` (no tsim_program involved):
 *   row_ptr   int32 [n_out + 1], row_ptr[0] = 0, non-decreasing;  cols  int32 [row_ptr[n_out]], each in [0, M);
 *   ref       uint8 [n_out], 0/1 (the noiseless value of each output; zeros for skip_reference_sample).
 * Any M: the records' 64-bit shot masks live in LDS, in windows of 2048 records when M exceeds 7616 (each window
 * with its own CSR, built here); TSIM_ENOTSUP only when the windows' CSRs would exceed 2^28 row pointers.
 * Rows: input row r starts at byte r * in_row_bytes and holds M bytes (in_packed = 0: nonzero = 1) or ceil(M/8) bytes
 * little-endian (in_packed = 1; pad bits ignored) - the padded uint64 rows of tsim_sample_steps_device qualify with
 * in_row_bytes = 8 ceil(M/64).  The input buffer must span B * in_row_bytes bytes: whole rows, the last one included,
 * may be read.  Output row r starts at byte r * out_row_bytes and receives outputs col0 .. col0+n_cols-1 as
 * n_cols bytes 0/1 (out_packed = 0) or ceil(n_cols/8) bytes with zero pad bits (out_packed = 1); the bytes of a row past
 * those are not written. */
typedef struct tsim_m2d tsim_m2d;
int tsim_m2d_create(int32_t device, int32_t num_measurements, int32_t n_out, const int32_t *row_ptr, const int32_t *cols,
                    const uint8_t *ref, tsim_m2d **out);
void tsim_m2d_destroy(tsim_m2d *h);
/* host arrays: chunked H2D -> kernel -> D2H through pinned staging owned by the handle (device memory bounded for any B);
 * synchronous.  out_row_bytes bytes of every output row are copied back. */
int tsim_m2d_convert(tsim_m2d *h, const uint8_t *meas, int64_t B, int64_t in_row_bytes, int32_t in_packed, uint8_t *out,
                     int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols);
/* device buffers owned by the caller, asynchronous on `stream` (NULL: the handle's own stream) */
int tsim_m2d_convert_device(tsim_m2d *h, const uint8_t *d_meas, int64_t B, int64_t in_row_bytes, int32_t in_packed,
                            uint8_t *d_out, int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols,
                            void *stream);
/* out[0] num_measurements, [1] n_out, [2] nnz, [3] device */
int tsim_m2d_info(const tsim_m2d *h, int64_t out[4]);

/* ---- affine measurement sampler (CliffordCircuit.compile_sampler(method="affine")) ---------------------------------------
 * Every measurement record of a Clifford circuit with Pauli noise is an affine GF(2) function of the error bits and of
 * independent uniform bits.  Per shot n, output j = flip[j] XOR (XOR of x[cols[k]] over k in row_ptr[j] .. row_ptr[j+1]-1);
 * a column listed twice cancels.  Columns 0 <= c < num_f are bit c of the shot's packed f row (little-endian bits, rows
 * f_row_bytes apart, as tsim_noise_sample_device writes them; num_f = 0 allows d_f = NULL).  Columns num_f <= c <
 * num_f + n_random are random symbol s = c - num_f: with g = first_shot + n, (x0, x1) = threefry2x32((key_hi, key_lo),
 * counter (s, g / 64)) and w = x0 | x1 << 32, the symbol's value is bit g % 64 of w.  first_shot must be a multiple of 64
 * and first_shot + B at most 2^38; results depend on the key and on g only, not on how a request is cut into launches.
 * A handle of its own, bound to HIP device `device`; every argument is checked before any device call (TSIM_EINVAL).
 * Output rows follow tsim_m2d_convert_device: row r at byte r * out_row_bytes receives outputs col0 .. col0+n_cols-1 as
 * n_cols bytes 0/1 (out_packed = 0) or ceil(n_cols/8) bytes with zero pad bits (out_packed = 1); the bytes of a row past
 * those are not written.  Asynchronous on `stream` (NULL: the handle's own stream). */
typedef struct tsim_affine tsim_affine;
int tsim_affine_create(int32_t device, int32_t num_f, int32_t n_random, int32_t n_out, const int32_t *row_ptr,
                       const int32_t *cols, const uint8_t *flip, tsim_affine **out);
void tsim_affine_destroy(tsim_affine *h);
int tsim_affine_sample_device(tsim_affine *h, const uint64_t *d_f, int64_t f_row_bytes, int64_t B, int64_t first_shot,
                              uint32_t key_hi, uint32_t key_lo, uint8_t *d_out, int64_t out_row_bytes, int32_t out_packed,
                              int32_t col0, int32_t n_cols, void *stream);
/* out[0] num_f, [1] n_random, [2] n_out, [3] nnz, [4] device, [5] columns per window, [6] windows, [7] LDS bytes per wave */
int tsim_affine_info(const tsim_affine *h, int64_t out[8]);

/* ---- Pauli-frame sampler (CliffordCircuit.compile_sampler / compile_detector_sampler(method="frame")) ----------------------
 * A Pauli frame (x_q, z_q) per shot is carried through the circuit, 64 shots to a word; noise is drawn where it acts.  The
 * compiled form (tsim_amd/frame.py documents it and states the same function in numpy):
 *   operations  op_kind uint8 [n_ops] (0 H, 1 S, 2 CX, 3 RESET, 4 MEASURE, 5 FEEDBACK, 6 NOISE), op_a / op_b / op_c int32:
 *               H/S/RESET a = qubit; CX a = control, b = target; MEASURE a = qubit or -1 (the flip word is zero), b = record;
 *               FEEDBACK a = record, b = qubit, c = 1 (into x) | 2 (into z); NOISE a = site;
 *   batches     batch_ptr int32 [n_batches + 1]: operations of one kind whose qubits and records are pairwise disjoint;
 *   sites       site_chan (the index folded into the site's key), site_table int32 [n_sites], site_bit int32 [n_sites + 1]
 *               (the site's error bits, 1 .. 32 of them), bit_ptr int32 [n_bits + 1] (targets of an error bit), targets
 *               int32 [n_targets] = 4 * index + kind (0 x of qubit, 1 z of qubit, 2 record);
 *   tables      table_ptr int32 [n_tables + 1], table_gap int32 [n_tables], out_vals / out_thr uint32 [n_outcomes] (the
 *               outcome's error bits; ceil(cdf 2^32), non-decreasing), gap_thr uint32 [n_gaps][64] (floor((1-p)^k 2^32),
 *               k = 1 .. 64);
 *   outputs     out_const uint8 [n_out], out_ptr int32 [n_out + 1], out_cols int32 [n_cols] over the columns
 *               [n_records records | n_random random symbols]; records n_records .. n_records + n_hidden - 1 are scratch.
 * Per shot g = first_shot + n, output j = out_const[j] XOR its records' flips XOR its symbols; symbol s is bit g % 64 of
 * x0 | x1 << 32 of threefry2x32((key_hi, key_lo), (s, g / 64)) as in tsim_affine_sample_device; site n draws under
 * (n0 ^ site_chan[n] * 0x9E3779B9, n1) with (n0, n1) = threefry2x32(key, (0x6E6F6973, 0x6672616D)), counter (g / 64, draw).
 * Results depend on the key and on g only.  n_qubits (16 bytes of LDS per qubit and word) above 10240 is TSIM_ENOTSUP at create
 * time; every index of the form is checked there, before any device call.  The handle owns the record-flip scratch (at most
 * 256 MiB) and cuts a request into launches that fit it; launches of one handle must be ordered (one stream at a time).
 * Output rows, col0 / n_cols, first_shot and stream: as tsim_affine_sample_device. */
typedef struct tsim_frame_desc {
  int32_t n_qubits, n_records, n_hidden, n_random, n_out, n_ops, n_batches, n_sites, n_bits, n_targets, n_tables, n_outcomes,
      n_gaps, n_cols;
  const uint8_t *op_kind;
  const int32_t *op_a, *op_b, *op_c, *batch_ptr;
  const int32_t *site_chan, *site_table, *site_bit, *bit_ptr, *targets, *table_ptr, *table_gap;
  const uint32_t *out_vals, *out_thr, *gap_thr;
  const uint8_t *out_const;
  const int32_t *out_ptr, *out_cols;
} tsim_frame_desc;
typedef struct tsim_frame tsim_frame;
int tsim_frame_create(int32_t device, const tsim_frame_desc *desc, tsim_frame **out);
void tsim_frame_destroy(tsim_frame *h);
int tsim_frame_sample_device(tsim_frame *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
                             int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols, void *stream);
/* out[0] n_qubits, [1] n_records, [2] n_hidden, [3] n_random, [4] n_out, [5] n_ops, [6] n_batches, [7] n_sites, [8] device,
 * [9] T (64-shot words per block of k_frame), [10] LDS bytes of its frames, [11] the most qubits a handle takes, [12] columns
 * per window of the output stage, [13] its windows, [14] words per launch, [15] items of the largest batch */
int tsim_frame_info(const tsim_frame *h, int64_t out[16]);

/* ---- fault-driven detector sampler (CliffordCircuit.compile_detector_sampler(method="faults")) ----------------------------
 * Every deterministic detector and observable is a constant XOR some error bits: a shot draws which noise sites fire, by
 * geometric skipping over the sites that share one outcome table, and XORs each fired error bit's list of outputs into its
 * row.  The compiled form (tsim_amd/faults.py documents it and states the same function in numpy):
 *   classes     class_ptr int32 [n_classes + 1]: the sites of class c (they share table c), site_e0 int32 [n_sites] (class-
 *               major: the site's first error bit), table_bits int32 [n_classes] (error bits per site, 1 .. 32);
 *   tables      table_ptr int32 [n_classes + 1], table_gap int32 [n_classes], out_vals / out_thr uint32 [n_outcomes] (the
 *               outcome's error bits; ceil(cdf 2^32), non-decreasing), gap_thr uint32 [n_gaps][gap_k] (floor((1-p)^k 2^32),
 *               k = 1 .. gap_k, non-increasing; gap_k must be 1024, a constant of the stream);
 *   columns     col_ptr int32 [num_e + 1], cols int32 [n_cols]: the outputs error bit e flips; out_const uint8 [n_out].
 * Per shot g = first_shot + n and class c of n_c sites: key (n0 ^ c * 0x9E3779B9, n1) with (n0, n1) = threefry2x32(key,
 * (0x6E6F6973, 0x66616C74)); pos = -1; draw j: (x0, x1) = threefry2x32(class key, (g mod 2^32, (g >> 32) | (j << 6)));
 * skip = #{k : x0 < gap_thr[k]}; skip == gap_k: pos += gap_k and draw again; else pos += skip + 1, the class is done when
 * pos >= n_c, else site pos fires with the first outcome whose threshold exceeds x1 (the last one when none does).  Results
 * depend on the key and on g only.  A class of more than 2^25 sites (the draw index has 26 bits) is TSIM_ENOTSUP at create
 * time; every index, CSR pointer, threshold order and size of the form is checked there, before any device call.  The handle
 * owns no scratch: a request is one launch, rows live in LDS (outputs beyond one wave's LDS, about 20 000, go through in
 * column windows that redraw the stream).  Output rows, col0 / n_cols, first_shot and stream: as tsim_frame_sample_device. */
typedef struct tsim_faults_desc {
  int32_t n_out, num_e, n_sites, n_classes, n_outcomes, n_gaps, gap_k, n_cols;
  const int32_t *class_ptr, *site_e0, *table_bits, *table_ptr, *table_gap;
  const uint32_t *out_vals, *out_thr, *gap_thr;
  const int32_t *col_ptr, *cols;
  const uint8_t *out_const;
} tsim_faults_desc;
typedef struct tsim_faults tsim_faults;
int tsim_faults_create(int32_t device, const tsim_faults_desc *desc, tsim_faults **out);
void tsim_faults_destroy(tsim_faults *h);
int tsim_faults_sample_device(tsim_faults *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
                              int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols, void *stream);
/* out[0] n_out, [1] num_e, [2] n_sites, [3] n_classes, [4] device, [5] gap_k, [6] columns per window, [7] windows of all
 * outputs, [8] 32-bit words per LDS row, [9] waves per block, [10] LDS bytes per block, [11] 1 when the tables live in LDS,
 * [12] n_gaps, [13] n_cols, [14] sites of the largest class, [15] the most columns a window can have */
int tsim_faults_info(const tsim_faults *h, int64_t out[16]);

/* ---- fixed-weight fault sampling (compile_detector_sampler(method="faults", fault_weight=k)) on the same handle ------------
 * Rows conditioned on exactly k noise sites firing: the strata of a stratified logical error rate (tsim_amd/fixed_weight.py
 * documents the law and states the same function in numpy).  tsim_faults_set_split uploads the table of the class counts,
 * split_thr uint32 [n_classes][kmax + 1][kmax + 1] (host array): row (c, r) is ceil(cdf 2^32) of P(class c takes m of the r
 * sites still to place in the classes c, c + 1, ...), entries from min(r, n_c) upward 2^32 - 1; one table serves every
 * k <= kmax.  Checked before any device call: kmax in 0 .. 32 and a non-NULL table, rows that do not decrease, and in every
 * row a split can reach a zero wherever m would leave the later classes more sites than they hold (TSIM_EINVAL); a class
 * with an all-zero gap row (p_fire = 1: no odds) is TSIM_ENOTSUP.  A second call replaces the table.
 * tsim_faults_sample_weight_device has the contract of tsim_faults_sample_device (rows, col0 / n_cols, first_shot, stream,
 * one launch, results a function of the key, k and g only).  Per shot g, r = k, the classes in order under the class keys of
 * the noise key threefry2x32(key, (0x6E6F6973, 0x66697877)): draw 0 of class c, x0, picks k_c = the smallest m < min(r, n_c)
 * with x0 < thr[m] of row (c, r), min(r, n_c) when there is none (the last class takes r without a draw), r -= k_c; draws
 * j = 1, 2, ...: t = x0 n_c, pos = t >> 32, rejected when t mod 2^32 < 2^32 mod n_c or pos fired already in this shot and
 * class, else site pos fires with the first outcome whose threshold exceeds x1; until k_c sites have fired.  k < 0, k > kmax
 * and k > n_sites are TSIM_EINVAL, a call without a split table is TSIM_ESTATE. */
int tsim_faults_set_split(tsim_faults *h, int32_t kmax, const uint32_t *split_thr);
int tsim_faults_sample_weight_device(tsim_faults *h, int32_t k, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo,
                                     uint8_t *d_out, int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols,
                                     void *stream);
/* out[0] kmax of the split table (-1: none, the rest then 0), [1] waves per block, [2] LDS bytes per block (tables, then per
 * wave its rows and 8 KiB of fired positions), [3] 1 when the outcome tables and the split table live in LDS (together at
 * most 32 KiB), [4] 32-bit words per LDS row, [5] columns per window, [6] windows of all outputs, [7] bytes of the table */
int tsim_faults_weight_info(const tsim_faults *h, int64_t out[8]);

/* ---- counts over bit-packed device rows (the samplers' count(): rates without moving the rows to the host) ---------------
 * Row r starts at byte r * row_bytes of d_rows and holds n_cols columns little-endian (row_bytes >= ceil(n_cols/8); the
 * buffer spans n * row_bytes bytes).  Optional rows of ceil(n_cols/8) bytes: d_xor is XORed into every row first, and a
 * row is KEPT iff (row ^ xor) & test == 0 (d_test NULL: every row is kept).  The pad bits of d_test (columns n_cols and up of
 * its last byte) MUST BE ZERO here: this entry point compares the mask's whole bytes, so a set pad bit tests a bit of the row
 * that is no column (the handles below cut the mask's pad bits away themselves).  ACCUMULATED into d_counts (uint64, 8-byte
 * aligned, never zeroed here; 2 + n_cols + 2^n_hist entries):
 *   [0] kept rows;  [1] kept rows with a set bit in columns obs_lo .. obs_hi - 1;  [2 + c] kept rows with column c set;
 *   [2 + n_cols + b] kept rows whose bits at hist_cols[0 .. n_hist-1] (host array, distinct columns, n_hist <= 16) spell
 *   b, bit i = column hist_cols[i].
 * Asynchronous on `stream` (NULL: the null stream) of HIP device `device`.  Arguments are checked before any launch;
 * n == 0 returns 0 without a launch. */
int tsim_tally_rows_device(int32_t device, const uint8_t *d_rows, int64_t n, int64_t row_bytes, int32_t n_cols,
                           const uint8_t *d_xor, const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, const int32_t *hist_cols,
                           int32_t n_hist, uint64_t *d_counts, void *stream);

/* ---- pair counts over bit-packed device rows (count(pair_columns=...): the matrix the p_ij correlation analysis of
 *      detection events is computed from) ---------------------------------------------------------------------------
 * N[a][b] = kept rows with columns pair_cols[a] and pair_cols[b] both set, for all ordered pairs of n_pair selected
 * columns (1 .. 4096 of them, distinct, any order, each in 0 .. n_cols-1): a binary X^T X, exact uint64.  Rows, d_xor and
 * d_test are those of tsim_tally_rows_device and mean the same: a row is KEPT iff (row ^ xor) & test == 0, the counts are
 * taken over row ^ xor, so N[a][a] is the tally's count of column pair_cols[a]; pad bits and padding bytes of the rows
 * are never counted.  A handle of its own, bound to HIP device `device` (no tsim_program involved): it owns the column
 * list, the n_pair x n_pair counters (zero after create) and the bit-plane workspace of one slab of rows (at most
 * 32 MiB; a slab is 2^16 .. 2^20 rows).  Arguments are checked before any device call. */
typedef struct tsim_pairs tsim_pairs;
int tsim_pairs_create(int32_t device, int32_t n_cols, const int32_t *pair_cols, int32_t n_pair, tsim_pairs **out);
void tsim_pairs_destroy(tsim_pairs *h);
/* ACCUMULATES the counts of n rows, slab by slab (two launches each); asynchronous on `stream` (NULL: the null stream).
 * The launches share the handle's workspace: calls on one handle go to one stream, or are ordered by the caller.
 * n == 0 returns 0 without a launch. */
int tsim_pairs_add_device(tsim_pairs *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                          const uint8_t *d_test, void *stream);
/* the counters as the full symmetric matrix, out[a * n_pair + b] (host array); enqueued behind the work of `stream`, which
 * is synchronised */
int tsim_pairs_read(tsim_pairs *h, uint64_t *out, void *stream);
/* zeroes the counters, asynchronous on `stream` */
int tsim_pairs_reset(tsim_pairs *h, void *stream);
/* out[0] n_pair, [1] workspace bytes, [2] rows per slab, [3] kernel launches so far */
int tsim_pairs_info(const tsim_pairs *h, int64_t out[4]);

/* ---- pattern counts over bit-packed device rows (count(pattern_columns=...): which whole patterns occurred, how often)
 *      and the lookup decoder built from them (count(decoder=...)) ---------------------------------------------------
 * The distinct patterns of the kept rows, each with its exact uint64 count.  Rows, d_xor and d_test are those of
 * tsim_tally_rows_device and mean the same: a row is KEPT iff (row ^ xor) & test == 0, and its pattern is row ^ xor at
 * the n_key key columns (distinct, any order, each in 0 .. n_cols-1; no limit but memory), bit i of the pattern = column
 * key_cols[i]; pad bits and padding bytes of the rows never belong to a pattern.  A handle of its own, bound to HIP
 * device `device`: an open-addressing table of `capacity` slots (1 .. 2^30, rounded up to a power of two; 16 bytes per
 * slot for n_key <= 63, 16 + 8 * ceil(n_key / 64) otherwise, 8 more once tsim_rowtab_load gave it values), zero after
 * create.  Keys of at most 63 bits are the compared-and-swapped word themselves; wider keys are found by a 63-bit
 * fingerprint, and EVERY kept row's full key is then compared with the key its slot stores (a second launch): a
 * mismatch is counted (info [5]) and makes tsim_rowtab_read fail - a count is exact or the call says so.  A row whose
 * pattern is absent and finds no empty slot within min(capacity, 1024) probes is counted as OVERFLOW (info [4]) and
 * dropped; slots are never freed, so every pattern in the table carries its full count and
 * sum(counts) + overflow == kept at all times.  Arguments are checked before any device call. */
typedef struct tsim_rowtab tsim_rowtab;
int tsim_rowtab_create(int32_t device, int32_t n_cols, const int32_t *key_cols, int32_t n_key, int64_t capacity, tsim_rowtab **out);
void tsim_rowtab_destroy(tsim_rowtab *h);
/* ACCUMULATES n rows into the table (one launch; two for keys wider than 63 bits); asynchronous on `stream` (NULL: the
 * null stream).  Calls on one handle go to one stream, or are ordered by the caller.  n == 0 returns 0 without a launch. */
int tsim_rowtab_add_device(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                           const uint8_t *d_test, void *stream);
/* the entries, in slot order: keys_out[e * ceil(n_key/8) ..] the pattern bit-packed little-endian over the key columns in
 * the order given at create, counts_out[e] its rows (host arrays with room for max_entries); *n_entries: how many there
 * are (TSIM_EINVAL when more than max_entries - *n_entries is set all the same).  Enqueued behind the work of `stream`,
 * which is synchronised.  TSIM_ESTATE when a fingerprint collision was met: nothing is returned. */
int tsim_rowtab_read(tsim_rowtab *h, uint8_t *keys_out, uint64_t *counts_out, int64_t max_entries, int64_t *n_entries, void *stream);
/* empties the table and zeroes its counters, asynchronous on `stream` */
int tsim_rowtab_reset(tsim_rowtab *h, void *stream);
/* out[0] capacity, [1] distinct entries, [2] rows added, [3] rows kept, [4] overflow rows, [5] unresolved collisions
 * (rows whose key differs from the key of the slot their fingerprint leads to), [6] kernel launches so far, [7] bytes
 * of device memory.  Synchronises the device. */
int tsim_rowtab_info(tsim_rowtab *h, int64_t out[8]);
/* The lookup decoder.  tsim_rowtab_load replaces the table's contents by n distinct keys (host array, laid out as
 * keys_out of tsim_rowtab_read) with one 8-byte value each (synchronous; TSIM_ENOTSUP when a key finds no slot).
 * tsim_rowtab_decode_device then looks every kept row's key up, read-only (full keys compared), XORs the slot's value
 * (0 for a key that is not in the table) with the row's columns obs_lo .. obs_hi - 1 (at most 64; bit i = column
 * obs_lo + i) and ACCUMULATES into d_counters (uint64[3], 8-byte aligned, never zeroed here): [0] kept rows, [1] kept
 * rows whose value differs from their observables, [2] kept rows whose key is not in the table.  Asynchronous on
 * `stream`; TSIM_ESTATE before a load. */
int tsim_rowtab_load(tsim_rowtab *h, const uint8_t *keys, const uint64_t *values, int64_t n);
int tsim_rowtab_decode_device(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                              const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, void *stream);
/* tsim_rowtab_decode_device with an outlet for the predictions: every argument means the same and accumulates the same, and
 * d_pred (uint64[n], 8-byte aligned) receives every row's value under the contract of tsim_uf_decode_device's d_pred: 0 for a
 * row that is not kept and for a key that is not in the table.  d_pred == NULL is tsim_rowtab_decode_device itself. */
int tsim_rowtab_decode_pred_device(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                   const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                   void *stream);

/* ---- predictions into bit-packed device rows (count(decoder=..., corrected=True): corrected observables; decode_file) -----
 * d_pred[r] (uint64[n], 8-byte aligned: the d_pred of a decode call below or above) is the prediction of row r, bit k =
 * column col0 + k, for n_obs columns (1 .. 64; the bits at and above n_obs are ignored); rows as for tsim_tally_rows_device
 * (any base address, any row_bytes >= 1), col0 >= 0 and col0 + n_obs <= 8 * row_bytes.
 *   mode 0 (XOR):   the columns col0 .. col0 + n_obs - 1 of row r become ^= bit k of d_pred[r].  No other bit of the buffer
 *                   changes, pad bits and padding bytes included, and a row whose prediction is 0 is not written at all: the
 *                   rows of a decode call become rows with CORRECTED observables, which every reader above takes unchanged.
 *   mode 1 (WRITE): the columns are SET to those bits and the other bits of the bytes col0 / 8 .. (col0 + n_obs - 1) / 8 are
 *                   cleared; bytes outside those are not touched.  With col0 = 0 and row_bytes = ceil(n_obs / 8) the buffer
 *                   becomes the rows of predictions the shot-data encoders take (tsim_shotdata_encode).
 * One lane per row, 8-byte accesses when d_rows and row_bytes are multiples of 8, bytes otherwise.  Asynchronous on `stream`
 * (NULL: the null stream) of HIP device `device`: behind the decode call that writes d_pred on the same stream it needs no
 * other ordering.  Arguments are checked before any device call (TSIM_EINVAL); n == 0 returns 0 without a launch. */
int tsim_pred_rows_device(int32_t device, const uint64_t *d_pred, int64_t n, int32_t n_obs, uint8_t *d_rows, int64_t row_bytes,
                          int32_t col0, int32_t mode, void *stream);

/* ---- the union-find (cluster-growth) decoder over bit-packed device rows (count(decoder=UnionFindDecoder)) ----------
 * The decoding graph: node 0 is the boundary, node i + 1 is detector (column) i; edge e joins edge_u[e] < edge_v[e], the
 * pairs strictly ascending, and flips the observables edge_obs[e] (bit k = observable k).  The rule - synchronous
 * growth rounds, the forest of smallest-index roots and parent edges, peeling - is the module docstring of
 * tsim_amd/decode.py; it fixes the prediction whatever the order of the lanes.  n_cols: the columns of the rows this
 * handle will be given (>= n_nodes - 1).  A handle of its own, bound to HIP device `device`.  tsim_uf_create checks every
 * index and the ordering before any device call (TSIM_EINVAL); TSIM_ENOTSUP for more than 65535 nodes or edges and when
 * one shot's state (8 bytes per node, 10 bytes per 32 edges) does not fit a block's 64 KiB of LDS. */
typedef struct tsim_uf tsim_uf;
typedef struct tsim_uf_desc {
  int32_t n_nodes, n_edges, n_cols;
  const int32_t *edge_u, *edge_v;
  const uint64_t *edge_obs;
} tsim_uf_desc;
int tsim_uf_create(int32_t device, const tsim_uf_desc *desc, tsim_uf **out);
/* Weighted growth: edge_cap[e] in 1 .. 14 is the growth an edge takes to be full (grown[e] = min(cap[e], grown[e] +
 * active ends) per round); edge_cap == NULL is tsim_uf_create, which is cap 2 everywhere.  A cap outside 1 .. 14 is
 * TSIM_EINVAL, checked with the other arguments before any device call.  A shot's state then holds 4 bits per edge in
 * the place of one of the two edge bitmaps (8 bytes per node, 6 + 16 bytes per 32 edges) for the 64 KiB limit. */
int tsim_uf_create_weighted(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, tsim_uf **out);
/* Heralded erasures (DecodingGraph.from_form(form, heralds=True)): a row has n_det_cols detector columns, of which
 * node_det[v - 1] (int32[n_nodes - 1], strictly ascending) is the column of node v and herald_det[i] (int32[n_heralds])
 * the column of herald i; every column is a node or one herald, so n_det_cols == n_nodes - 1 + n_heralds, and
 * desc->n_cols >= n_det_cols.  herald_edges[herald_ptr[i] .. herald_ptr[i + 1] - 1] (herald_ptr int32[n_heralds + 1] from 0,
 * never falling; an empty list is allowed, an edge may be listed under several heralds) are the edges that start FULL in a
 * row whose column herald_det[i] is set after d_xor.  A herald is no defect: a kept row whose node columns are all 0
 * predicts 0, is not decoded and does not count in out[7] of tsim_uf_info, whatever its heralds say.  Growth, forest and
 * peeling are those of the other handles; so are the state in LDS and its limits (heralds take no per-shot state and their
 * number is bounded by int32 only).  edge_cap: as tsim_uf_create_weighted, NULL for unweighted growth.  her == NULL is
 * tsim_uf_create_weighted.  Every column, the ordering, the lists and their edge indices are checked on the host before any
 * device call (TSIM_EINVAL). */
typedef struct tsim_uf_heralds {
  int32_t n_det_cols, n_heralds;
  const int32_t *node_det, *herald_det, *herald_ptr, *herald_edges;
} tsim_uf_heralds;
int tsim_uf_create_heralds(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her,
                           tsim_uf **out);
/* Cluster matching ("Cluster matching" in the module docstring of tsim_amd/decode.py): growth as the other handles (edge_cap
 * as tsim_uf_create_weighted, NULL: cap 2 everywhere), then every cluster of 1 .. max_defects defects is corrected by the
 * minimum-weight matching of its defects, the boundary allowed, under the match weights match_w[e] in 1 .. 65535
 * (uint16[n_edges], required), by a dynamic program over the subsets of its defects with the tie rule of the docstring; a
 * larger cluster is peeled as before.  The distances and the observables of the paths come from the match table
 * (uint32 + uint64 per pair of nodes), which this call builds on the device.  max_defects is 1 .. 12.  No heralds: the
 * table is static.  Every argument - the graph as tsim_uf_create, the caps, a NULL match_w, a weight of 0, max_defects - is
 * checked before any device call (TSIM_EINVAL).  TSIM_ENOTSUP for more than 2048 nodes and when a shot's state plus the
 * dynamic program's (5 bytes per subset: 2^max_defects subsets; 4 bytes per pair of a cluster's defects) does not fit a
 * block's 64 KiB of LDS.  tsim_uf_decode_device on the handle runs the matching kernel and means what it means on the
 * others; tsim_uf_decode_soft_device is TSIM_EINVAL. */
int tsim_uf_create_matching(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const uint16_t *match_w,
                            int32_t max_defects, tsim_uf **out);
/* The match table of a handle of tsim_uf_create_matching, to the host: dist (uint32[n_nodes * n_nodes], 0x7FFFFFFF: no path)
 * and mask (uint64[n_nodes * n_nodes]), row a = source a.  TSIM_EINVAL for another handle or a NULL.  Synchronous. */
int tsim_uf_match_table(tsim_uf *h, uint32_t *dist, uint64_t *mask);
/* Cluster matching with the complementary gap of one observable ("Complementary gap" in the module docstring of
 * tsim_amd/decode.py): everything tsim_uf_create_matching does, then the class table dist2 (uint32[n_nodes * n_nodes * 2]:
 * per pair of nodes the least weight of a walk whose bit `observable` of edge_obs XORs to 0, and to 1; 8 bytes per pair, 32 MB
 * at 2048 nodes) is built on the device and W0, the lightest logical without a defect, is taken from it.  observable is
 * 0 .. 63 (TSIM_EINVAL), checked with every other argument before any device call.  A shot's state holds both dynamic
 * programs (13 bytes per subset, 12 bytes per pair of a cluster's defects): TSIM_ENOTSUP when it does not fit a block's
 * 64 KiB of LDS.  tsim_uf_decode_device on the handle decodes as on a handle of tsim_uf_create_matching, tsim_uf_info [13] ..
 * [15] mean the same, tsim_uf_decode_soft_device is TSIM_EINVAL; tsim_uf_decode_gap_device is the call it adds. */
int tsim_uf_create_matching_gap(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const uint16_t *match_w,
                                int32_t max_defects, int32_t observable, tsim_uf **out);
/* The class table of a handle of tsim_uf_create_matching_gap, to the host: dist2[(a * n_nodes + v) * 2 + b] (0x7FFFFFFF: no
 * walk), and *w0 = W0, -1 when no source reaches the boundary in both classes.  TSIM_EINVAL for another handle or a NULL.
 * Synchronous. */
int tsim_uf_gap_table(tsim_uf *h, uint32_t *dist2, int64_t *w0);
/* Cluster matching for a graph with heralds ("Cluster matching under heralds" in the module docstring of tsim_amd/decode.py):
 * growth as tsim_uf_create_heralds, the match table (and, with observable >= 0, the class table and W0) as
 * tsim_uf_create_matching(_gap) over the nodes and edges of the herald graph.  A cluster of 1 .. max_defects defects whose hub
 * graph - its defects and the other non-boundary ends of its erased edges - has at most max_hubs hubs is corrected by the
 * minimum-weight matching of its defects in that graph, where an erased edge e of the cluster weighs min(match_w[e], erased_w);
 * every other cluster is peeled.  her is required (a graph without heralds: tsim_uf_create_matching), max_defects is 1 .. 12,
 * erased_w 1 .. 65535, max_hubs max_defects .. 32, observable 0 .. 63 or -1 for a handle without the gap: all checked with the
 * graph, the caps, the heralds and the weights before any device call (TSIM_EINVAL).  TSIM_ENOTSUP for more than 2048 nodes and
 * when a shot's state - that of tsim_uf_create_matching(_gap) and the hub graph's, 12 bytes per pair of hubs, 20 with the gap -
 * does not fit a block's 64 KiB of LDS.  tsim_uf_decode_device takes the handle, tsim_uf_decode_gap_device one with an
 * observable, tsim_uf_decode_soft_device is TSIM_EINVAL; tsim_uf_info [13] .. [15] mean what they mean on a matching handle (a
 * cluster peeled for its hubs counts as peeled), tsim_uf_match_table and tsim_uf_gap_table give its tables. */
int tsim_uf_create_matching_heralds(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her,
                                    const uint16_t *match_w, int32_t max_defects, int32_t erased_w, int32_t max_hubs,
                                    int32_t observable, tsim_uf **out);
/* Of a handle of tsim_uf_create_matching_heralds (TSIM_EINVAL for another): out[0] erased_w, [1] max_hubs, [2] the matched
 * clusters that had an erased edge, [3] the clusters of at most max_defects defects that were peeled for having more than
 * max_hubs hubs, both over the rows decoded in LDS that are no miss.  Synchronises the device. */
int tsim_uf_erasure_info(tsim_uf *h, int64_t out[4]);
void tsim_uf_destroy(tsim_uf *h);
/* out[0] nodes, [1] edges, [2] LDS bytes per shot, [3] shots (waves) per block, [4] kernel launches so far, [5] the most
 * growth rounds a row took, [6] bytes of device memory, [7] rows decoded in LDS (kept rows with a defect), [8] n_cols,
 * [9] blocks of a full grid, [10] the largest cap (0: an unweighted handle), [11] heralds, [12] detector columns of a row
 * (n_nodes - 1 without heralds), [13] max_defects (0: not a handle of tsim_uf_create_matching), [14] clusters matched and
 * [15] clusters peeled, over the rows decoded in LDS that are no miss.  Synchronises the device. */
int tsim_uf_info(tsim_uf *h, int64_t out[16]);
/* Rows, d_xor, d_test, obs_lo, obs_hi and d_counters are those of tsim_rowtab_decode_device and mean the same (masks of
 * ceil(n_cols / 8) bytes): a row is KEPT iff (row ^ xor) & test == 0, its syndrome is row ^ xor at columns
 * 0 .. n_nodes - 2 (with heralds: at the columns node_det, the heralds at herald_det), the prediction is compared with its columns obs_lo .. obs_hi - 1, and the call ACCUMULATES into
 * d_counters: [0] kept rows, [1] kept rows whose prediction differs from their observables, [2] kept rows that are a
 * miss (growth stopped with an active cluster left: no flip is predicted).  d_pred (NULL: not wanted; 8-byte aligned)
 * receives every row's prediction as uint64[n]: 0 for a row that is not kept, and for a miss.  Asynchronous on `stream`;
 * calls on one handle go to one stream, or are ordered by the caller.  n == 0 returns 0 without a launch. */
int tsim_uf_decode_device(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                          const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                          void *stream);
/* tsim_uf_decode_device with the decoder's soft outputs ("Soft outputs" in the module docstring of tsim_amd/decode.py).
 * Everything up to d_pred means the same and accumulates the same.  Four values per row, from the state in which growth
 * ends (a miss included): [0] rounds, [1] full_edges, [2] largest_cluster, [3] correction_weight (0 for a miss); all four are
 * 0 for a row that is not kept and for a kept row without a defect.  metric (0 .. 3, in that order) is the value that is
 * binned, into n_bins (2 .. 1024) bins: the bin of x is min(x, n_bins - 1).  d_hist (uint64[2 * n_bins], 8-byte aligned,
 * required, never zeroed here): [b] ACCUMULATES the kept rows of bin b, [n_bins + b] those of them whose prediction differs
 * from their observables.  d_soft: NULL, or uint32[4 * n] (16-byte aligned) for the four values of every row.  Every kind
 * of handle takes it (plain, weighted, heralds); a shot's state in LDS and the limits of tsim_uf_create are unchanged.  A bad
 * metric or n_bins, or a NULL d_hist, is TSIM_EINVAL before any device call; n == 0 returns 0 without a launch; the
 * launches count in out[4] of tsim_uf_info. */
int tsim_uf_decode_soft_device(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                               const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                               int32_t metric, int32_t n_bins, uint64_t *d_hist, uint32_t *d_soft, void *stream);
/* tsim_uf_decode_device by a handle of tsim_uf_create_matching_gap, with the complementary gap of every row.  Everything up to
 * d_pred means the same and accumulates the same; the predictions are those of tsim_uf_decode_device.  A kept row with a
 * defect that is no miss has gap = min(gap_cap, the least gap of its clusters): |g0 - g1| of a matched cluster whose two
 * classes are finite, gap_cap when one is, 0 for a peeled cluster; a miss has gap 0.  The DEFICIT of a row is gap_cap - gap,
 * 0 for a row that is not kept and for a kept row without a defect; its bin is min(deficit / gap_step, n_bins - 1).  d_hist
 * (uint64[2 * n_bins], 8-byte aligned, required, never zeroed here) ACCUMULATES as the soft call's; d_gap: NULL, or
 * uint32[n] for the deficits.  gap_cap and gap_step are 1 .. 2^31 - 2, n_bins 2 .. 1024: a bad one, a NULL d_hist or another
 * kind of handle is TSIM_EINVAL before any device call; n == 0 returns 0 without a launch. */
int tsim_uf_decode_gap_device(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                              const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                              int64_t gap_cap, int64_t gap_step, int32_t n_bins, uint64_t *d_hist, uint32_t *d_gap, void *stream);

/* ---- sliding-window union-find decoding of long runs (count(decoder=WindowedUnionFindDecoder)) -----------------------
 * `global` is a decoding graph as above without heralds (with heralds: tsim_ufw_create_heralds below), bounded by int32 only; edge_cap as tsim_uf_create_weighted (NULL:
 * cap 2 everywhere); commit = C >= 1 and window = W > C are in detector columns.  The rule - the windows [k C, k C + W),
 * the validity condition, the window graphs with their open future boundary, merged pairs, local edge order and COMMITTED
 * edges, and a row decoded window after window with the committed flips carried on - is "Sliding-window decoding of long
 * runs" in the module docstring of tsim_amd/decode.py; it fixes the prediction whatever the order of the lanes.  The
 * library builds the windows itself, on the host.  Every index, the ordering, the caps and the validity condition (an edge
 * whose upper end lies past the window that commits its lower end: the buffer W - C is too small) are checked before any
 * device call (TSIM_EINVAL).  TSIM_ENOTSUP when a window has more than 65535 nodes or edges, and when one shot's state -
 * that of tsim_uf_create / _weighted for the largest window, a carry bitmap of the smallest power of two >= W bits and 16
 * bytes - does not fit a block's 64 KiB of LDS. */
typedef struct tsim_ufw tsim_ufw;
int tsim_ufw_create(int32_t device, const tsim_uf_desc *global, const uint8_t *edge_cap, int32_t commit, int32_t window,
                    tsim_ufw **out);
/* Sliding windows over a graph with heralds ("Sliding windows with heralds" in the same docstring).  `her` is the struct of
 * tsim_uf_create_heralds and means the same: a row has her->n_det_cols detector columns, node v sits in column
 * node_det[v - 1], herald i in column herald_det[i], and global->n_cols >= n_det_cols.  commit and window count NODES (the
 * non-herald detectors): the windows, the validity condition, the window graphs and the committed edges are those of
 * tsim_ufw_create over the nodes and edges of `global`; herald columns are never windowed.  In window k herald i lists the
 * distinct local edges of its global edges that are present there - an edge that leaves the window for the future as the
 * local boundary pair of its lower end - and in a row whose column herald_det[i] is set after d_xor those local edges start
 * FULL in that window.  The library builds these lists itself, on the host, with the windows.  A herald is no defect: "has
 * a defect", of a row and of a window, is taken from the node columns alone.  Everything tsim_ufw_create checks, and
 * everything tsim_uf_create_heralds checks of `her` (every column in range, node_det strictly ascending, each column a node
 * or exactly one herald, n_det_cols == n_nodes - 1 + n_heralds, herald_ptr from 0 and never falling, the edge indices), is
 * checked before any device call (TSIM_EINVAL).  TSIM_ENOTSUP as tsim_ufw_create: heralds take no per-shot LDS, their
 * tables lie in global memory.  her == NULL is tsim_ufw_create. */
int tsim_ufw_create_heralds(int32_t device, const tsim_uf_desc *global, const uint8_t *edge_cap, int32_t commit,
                            int32_t window, const tsim_uf_heralds *her, tsim_ufw **out);
/* Cluster matching in windows ("Cluster matching in windows" in the same docstring): everything tsim_ufw_create does, for a
 * graph without heralds, and in every decoded window that is no miss each cluster of 1 .. max_defects defects is corrected by
 * the minimum-weight matching of its defects in the window graph, the paths of the chosen pairs walked edge by edge so that
 * only their COMMITTED edges count; a larger cluster is peeled as before.  match_w (uint16[n_edges], required, 1 .. 65535) are
 * GLOBAL match weights: the weight of a local edge is the least among the global edges that land on it, computed on the host
 * beside the caps.  Per DISTINCT window - windows whose local arrays (nodes, edge_uv, edge_obs, weights, adjacency, commit
 * bitmap) are byte-identical share one - a match table of distances (uint32) and parent edges (uint16), 6 bytes per pair of
 * nodes and no masks, is built on the device by this call.  max_defects is 1 .. 12.  A NULL match_w, a weight of 0 and a bad
 * max_defects are TSIM_EINVAL, with everything tsim_ufw_create checks.  TSIM_ENOTSUP for a window of more than 2048 nodes, for
 * distinct tables of more than 1 GiB together, and when a shot's state - that of tsim_ufw_create, the dynamic program's of
 * tsim_uf_create_matching and 4 bytes per pair a cluster can choose - does not fit a block's 64 KiB of LDS.  All of it is
 * checked before any device call.  tsim_ufw_decode_device takes the handle and means what it means on the others;
 * tsim_ufw_decode_soft_device on it is TSIM_EINVAL. */
int tsim_ufw_create_matching(int32_t device, const tsim_uf_desc *global, const uint8_t *edge_cap, const uint16_t *match_w,
                             int32_t max_defects, int32_t commit, int32_t window, tsim_ufw **out);
/* The match table of window k of a handle of tsim_ufw_create_matching, to the host: dist (uint32[n * n], 0x7FFFFFFF: no path)
 * and parent (uint16[n * n]: the LOCAL parent edge of v from source a at [a * n + v], 0xFFFF for v == a and where there is no
 * path), n the nodes of window k.  TSIM_EINVAL for another handle, a NULL or a k outside the windows.  Synchronous. */
int tsim_ufw_match_table(tsim_ufw *h, int32_t k, uint32_t *dist, uint16_t *parent);
/* Of a handle of tsim_ufw_create_matching (TSIM_EINVAL for another; tsim_ufw_info has no free slot): out[0] max_defects,
 * [1] distinct match tables, [2] their bytes, [3] clusters matched and [4] clusters peeled, over the decoded windows of the
 * rows decoded in LDS that are no miss, [5] the most edges of a path walked, [6] and [7] zero.  Synchronises the device. */
int tsim_ufw_match_info(tsim_ufw *h, int64_t out[8]);
void tsim_ufw_destroy(tsim_ufw *h);
/* out[0] nodes and [1] edges of the global graph, [2] windows, [3] the most nodes and [4] the most edges of a window,
 * [5] LDS bytes per shot, [6] shots (waves) per block, [7] kernel launches so far, [8] the most growth rounds a window
 * took, [9] bytes of device memory, [10] rows decoded in LDS (kept rows with a defect on a node column), [11] windows
 * decoded (those with a defect, of such rows), [12] n_cols, [13] blocks of a full grid, [14] the largest cap (0:
 * unweighted), [15] heralds (0 for a handle of tsim_ufw_create).  That was the last free slot: the detector columns of a
 * row are out[0] - 1 + out[15] and have none of their own.  Synchronises the device. */
int tsim_ufw_info(tsim_ufw *h, int64_t out[16]);
/* The arguments of tsim_uf_decode_device, with the same meaning: kept / wrong / missed ACCUMULATE into d_counters, a row
 * with a miss in any window is a miss and predicts 0, d_pred is optional. */
int tsim_ufw_decode_device(tsim_ufw *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                           const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                           void *stream);
/* tsim_ufw_decode_device with the windowed decoder's soft outputs ("Soft outputs in windows" in the module docstring of
 * tsim_amd/decode.py); the contract is that of tsim_uf_decode_soft_device.  Everything up to d_pred means the same and
 * accumulates the same.  Four values per row, over its DECODED windows (those with a defect after the carries, in order, up to
 * and including one that misses): [0] rounds, the most of a window; [1] full_edges, the SUM of the windows' local edges that are
 * full when the window's growth ends (pre-grown and virtual ones included; an edge two windows fill counts twice);
 * [2] largest_cluster, the MAXIMUM of the windows' largest clusters; [3] correction_weight, the committed flips, 0 for a miss.
 * All four are 0 for a row that is not kept and for a kept row without a defect on a node column.  metric (0 .. 3), n_bins
 * (2 .. 1024), d_hist (uint64[2 * n_bins], 8-byte aligned, required, ACCUMULATES, never zeroed here) and d_soft (NULL, or
 * uint32[4 * n], 16-byte aligned) as there: a bad metric or n_bins, or a NULL d_hist, is TSIM_EINVAL before any device call;
 * n == 0 returns 0 without a launch; the launches count in out[7] of tsim_ufw_info.  Both kinds of handle take it; a shot's
 * state in LDS, the shots of a block and the grid are those of tsim_ufw_decode_device. */
int tsim_ufw_decode_soft_device(tsim_ufw *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                int32_t metric, int32_t n_bins, uint64_t *d_hist, uint32_t *d_soft, void *stream);

/* ---- stim's shot-data formats on the device (stim.read_shot_data_file / write_shot_data_file, the samplers'
 *      sample_write, CompiledMeasurementsToDetectionEventsConverter.convert_file) ------------------------------------
 * format: 0 "01", 1 "b8", 2 "r8", 3 "ptb64", 4 "hits", 5 "dets" (layouts: tsim_amd/shotdata.py).  A handle of its own,
 * bound to HIP device `device` (no tsim_program involved): scan scratch, a result block, a stream (used when a call
 * passes stream NULL) and grow-only staging buffers for callers.
 * Rows: row r starts at byte r * row_bytes and holds n_bits columns little-endian (row_bytes >= ceil(n_bits/8)); the
 * padded uint64 rows of the samplers qualify.  dets needs num_m + num_d + num_o == n_bits (its M, D, L sections). */
typedef struct tsim_shotdata tsim_shotdata;
int tsim_shotdata_create(int32_t device, tsim_shotdata **out);
void tsim_shotdata_destroy(tsim_shotdata *h);
/* encode n rows into d_out (caller-owned device memory of out_cap bytes; 8-byte aligned for ptb64, whose n must be a
 * multiple of 64).  *out_bytes receives the encoded size (r8, hits, dets: a length pass and a scan, then ONE 8-byte
 * read, synchronous on `stream`).  Returns 0 when the bytes were written (asynchronously on `stream`), 1 when out_cap
 * is too small (nothing written: grow the buffer and call again), or a negative error. */
int tsim_shotdata_encode(tsim_shotdata *h, int32_t format, const uint8_t *d_rows, int64_t n, int64_t row_bytes, int32_t n_bits,
                         int32_t num_m, int32_t num_d, int32_t num_o, uint8_t *d_out, int64_t out_cap, int64_t *out_bytes,
                         void *stream);
/* decode a chunk of a file (n_in bytes at d_in, starting at a row boundary; is_final: the file ends with it) into at most
 * max_rows rows at d_rows (a multiple of 64 for ptb64).  result: [0] rows decoded, [1] bytes consumed (the next chunk
 * starts there: a partial last row is read again), [2] byte offset within the chunk of the first fault (-1: none), [3]
 * its kind (1 bad character, 2 01 line of the wrong length, 3 index outside its section, 4 unknown or missing dets
 * prefix, 5 r8 run past the row's end, 6 the file ends inside a row or group, 7 malformed token).  Synchronous; r8,
 * hits and dets zero rows 0 .. max_rows - 1 first and set bits with dword atomics (the row buffer must extend to the
 * next multiple of 4 bytes).  b8 and ptb64 need n_bits >= 1. */
int tsim_shotdata_decode(tsim_shotdata *h, int32_t format, const uint8_t *d_in, int64_t n_in, int32_t is_final, int32_t n_bits,
                         int32_t num_m, int32_t num_d, int32_t num_o, uint8_t *d_rows, int64_t row_bytes, int64_t max_rows,
                         int64_t result[4], void *stream);
/* staging owned by the handle: slot 0 .. 15 of device (pinned = 0) or pinned host (pinned = 1) memory of at least nbytes
 * (+16), grown on demand (contents are not kept when it grows) */
int tsim_shotdata_staging(tsim_shotdata *h, int32_t slot, int32_t pinned, int64_t nbytes, void **ptr);
/* hipMemcpyAsync of any direction on `stream`, and a synchronisation of `stream` (NULL: the handle's own) */
int tsim_shotdata_copy(tsim_shotdata *h, void *dst, const void *src, int64_t nbytes, void *stream);
int tsim_shotdata_synchronize(tsim_shotdata *h, void *stream);

/* ---- multi-GPU: RCCL over xGMI, issued by the library (no PyTorch) --------------------------------------
 *
 * The path shards over shots: rank r of R evaluates in-batch rows [r B/R, (r+1) B/R)
 * with shot_offset = r B/R; the Threefry counter is the global row index, so results do not depend on R and
 * no data-path exchange exists.  The one collective assembles the finished bit_packed rows.  The reference
 * has no multi-device path (src/tsim/sampler.py:310 uses jax.devices()[0]).
 *
 * One process per GPU.  Rank 0 makes a unique id, the host processes pass its 128 bytes to every rank by
 * any out-of-band channel (tsim_amd/dist.py: file or TCP rendezvous), every rank calls tsim_dist_init.
 * Collectives are asynchronous on `stream` (NULL: the communicator's own stream); order them after the
 * sampling kernels by passing the stream those ran on (tsim_get_stream / tsim_pipeline_lane_stream), or with
 * tsim_dist_stream_wait.
 *   tsim_dist_gather_rows   every rank sends nbytes; rank `root` receives world*nbytes, rank-major (ncclGather)
 *   tsim_dist_alltoall_rows chunk j of every rank's send buffer (nbytes_per_peer each) lands on rank j at
 *                           offset rank*nbytes_per_peer: a gather whose roots are spread over the node
 *   tsim_dist_allreduce_max / tsim_dist_barrier   host-value helpers (blocking) for timing harnesses       */
#define TSIM_DIST_ID_BYTES 128
typedef struct tsim_dist tsim_dist;
int tsim_dist_unique_id(uint8_t id[TSIM_DIST_ID_BYTES]);
int tsim_dist_init(int32_t device, const uint8_t id[TSIM_DIST_ID_BYTES], int32_t rank, int32_t world, tsim_dist **out);
void tsim_dist_destroy(tsim_dist *d);
int tsim_dist_info(const tsim_dist *d, int32_t *rank, int32_t *world);
int tsim_dist_gather_rows(tsim_dist *d, const void *d_send, int64_t nbytes, void *d_recv, int32_t root, void *stream);
int tsim_dist_alltoall_rows(tsim_dist *d, const void *d_send, void *d_recv, int64_t nbytes_per_peer, void *stream);
int tsim_dist_allreduce_max(tsim_dist *d, double *value);
int tsim_dist_barrier(tsim_dist *d);
/* make `waiting_stream` wait for the work queued so far on `signalling_stream` (NULL = the communicator's) */
int tsim_dist_stream_wait(tsim_dist *d, void *waiting_stream, void *signalling_stream);
/* Cross-stream ordering around a collective without draining anything: tsim_dist_mark records marker `mark`
 * (0 .. TSIM_DIST_MARKS-1) on `stream` - e.g. right after a gather was queued there - and
 * tsim_dist_wait_mark makes `stream` wait for that marker only (a marker never recorded is a no-op). */
#define TSIM_DIST_MARKS 8
int tsim_dist_mark(tsim_dist *d, int32_t mark, void *stream);
int tsim_dist_wait_mark(tsim_dist *d, int32_t mark, void *stream);
/* hipDeviceSynchronize on `device` (timing harnesses that must not depend on torch.cuda.synchronize) */
int tsim_device_synchronize(int32_t device);

/* ---- plumbing: memory, streams, timing (replaces utils/cuda_helpers.py:73-141) */

int tsim_device_count(int32_t *count);
/* free / total bytes of the handle's device (hipMemGetInfo): what the reference's batch sizing reads from
 * jax's memory_stats (src/tsim/sampler.py:308-320) */
int tsim_mem_info(tsim_program *p, int64_t *free_bytes, int64_t *total_bytes);
/* Buffers are owned by the handle: tsim_program_destroy frees whatever was not returned. */
int tsim_malloc_device(tsim_program *p, int64_t nbytes, void **d_ptr);
int tsim_free_device(tsim_program *p, void *d_ptr);
int tsim_malloc_pinned(int64_t nbytes, void **h_ptr);      /* hipHostMalloc   */
int tsim_free_pinned(void *h_ptr);
int tsim_memcpy_h2d(tsim_program *p, void *d_dst, const void *h_src, int64_t nbytes);
int tsim_memcpy_d2h(tsim_program *p, void *h_dst, const void *d_src, int64_t nbytes);
int tsim_synchronize(tsim_program *p);                      /* handle's stream */
/* Asynchronous variants on a caller-chosen stream (NULL: the handle's) and the matching wait: the end-to-end sampler
 * downloads finished batches while later ones are sampled (utils/cuda_helpers.py:105-141 copies once, at the end).
 * Pageable host memory is allowed; the call may then block until the copy is done. */
int tsim_memcpy_d2h_async(tsim_program *p, void *h_dst, const void *d_src, int64_t nbytes, void *stream);
int tsim_memcpy_h2d_async(tsim_program *p, void *d_dst, const void *h_src, int64_t nbytes, void *stream);
int tsim_stream_synchronize(tsim_program *p, void *stream);
/* Auxiliary hipStream_t owned by the handle (index 0 .. TSIM_AUX_STREAMS-1; created on first use): work beside the
 * sampling lanes - the device-side channel sampler, transfers. */
#define TSIM_AUX_STREAMS 4
int tsim_aux_stream(tsim_program *p, int32_t index, void **stream);
/* The pipeline slot the next batch of tsim_sample_steps_device will take (it rotates over all TSIM_PIPELINE_SLOTS): pass
 * it to tsim_sample_batch_device_end later to make a stream wait for exactly that batch. */
int tsim_pipeline_next_slot(tsim_program *p, int32_t *slot);
/* the handle's hipStream_t, e.g. to order a collective after the sampling kernel */
int tsim_get_stream(tsim_program *p, void **stream);

/* Host helper, no device involved: `new_key, subkey = jax.random.split(key)` for the threefry2x32
 * key layout (the once-per-batch split of sampler.py:399); out = {new_hi, new_lo, sub_hi, sub_lo}. */
void tsim_key_split(uint32_t key_hi, uint32_t key_lo, uint32_t out[4]);
/* The per-batch idiom of the reference's sample loop in one call (sampler.py:399-401):
 * `key, subkey = split(key)` then tsim_sample_batch_device_begin with `subkey`; key = {hi, lo} is
 * updated in place.  Saves a foreign-function round trip per batch for Python hosts. */
int tsim_sample_batch_device_begin_split(tsim_program *p, int32_t slot, const uint64_t *d_f, int64_t B,
                                         int32_t num_f, uint32_t key[2], int64_t shot_offset, uint64_t *d_out,
                                         float *d_max_norm_dev, void *stream, uint32_t flags);

/* SEVERAL consecutive batches of the reference's batch loop in one call (src/tsim/sampler.py:340-420: per batch
 * `key, subkey = split(key)`, sampler.py:399, then one sample_program, sampler.py:117-167).  For j < n_steps:
 * d_out[j] = sample_program(d_f[j], subkey_j) - exactly what n_steps calls of tsim_sample_batch_device_begin_split
 * on consecutive pipeline slots give, bit for bit; `key` = {hi, lo} is advanced n_steps times.  The call only
 * enqueues (slots rotate through all TSIM_PIPELINE_SLOTS; tsim_synchronize, or tsim_sample_batch_device_end on the
 * slots, completes the results); all batches share B, num_f, shot_offset and `flags` (TSIM_PIPE_*; the inputs are
 * ordered after the handle's stream unless TSIM_PIPE_INPUTS_READY).  d_max_norm_dev may be NULL, and so may its
 * entries.  Where the register first pass applies (f rows of at most 128 bits, at most 64 outputs and 16 compiled
 * outputs, pattern tables on, short hard-row lists) the first passes of up to 8 batches are ONE grid
 * (k_sample_lw_multi: no kernel boundary, no host call between batches, one ramp and one tail per group) and their
 * hard rows one k_sample4h_multi batch behind it; any other program or launch plan goes batch by batch through
 * tsim_sample_batch_device_begin.  TSIM_AMD_FUSED_STEPS=0 forces the latter, TSIM_AMD_FUSED_MAX caps a group. */
int tsim_sample_steps_device(tsim_program *p, int32_t n_steps, const uint64_t *const *d_f, int64_t B, int32_t num_f,
                             uint32_t key[2], int64_t shot_offset, void *const *d_out, float *const *d_max_norm_dev,
                             uint32_t flags);

/* HIP-event timing of the sampling kernel launches on the handle's stream.
 * on = 1: every kernel of a launch; on = 2: only the first kernel of a launch (the pattern-table
 * pass when tables are active) - timing events drain the queue they are recorded on, which costs
 * pipelined launches ~10 us per step when every side-stream kernel is bracketed.            */
int tsim_profile_enable(tsim_program *p, int32_t on);
/* Bracket only one launch in `every` (default 1): each timing event costs a queue drain.        */
int tsim_profile_set_sampling(tsim_program *p, int32_t every);
/* Sum of kernel durations (ms) and number of launches since the last reset;
 * synchronises the stream.                                                   */
int tsim_profile_read(tsim_program *p, double *kernel_ms, int64_t *launches, int32_t reset);
/* The same total split by kernel: [0] pattern-table pass (k_sample_lw), [1] hard-row kernel
 * (k_sample4h), [2] full kernel (k_sample4 / k_sample); call before a resetting tsim_profile_read. */
int tsim_profile_read_stages(tsim_program *p, double stage_ms[3]);
/* Batches covered by the bracketed first passes since the last reset: a fused first pass
 * (tsim_sample_steps_device) is ONE launch in tsim_profile_read that serves several batches. */
int tsim_profile_read_steps(tsim_program *p, int64_t *steps, int32_t reset);

/* ---- introspection ---------------------------------------------------- */

int tsim_program_info(const tsim_program *p, int32_t *n_components, int32_t *num_outputs,
                      int64_t *image_bytes, int64_t *total_graphs, int64_t *total_rows);

/* packer statistics: out[0] fast formulation selected, [1] levels, [2] fixed-frame levels,
 * [3] product pairs, [4] counted NodePhases rows, [5] table entries, [6] graphs with tabled
 * PhasePairs, [7] low 4 bits: full-evaluation kernel: 0 row kernel, 1 LDS chunk tables (k_sample4), 2 sparse columns for wide
 * components (k_sample4w); + 32: the program has a wide record (k_sample_wide serves it); + 16: with the shared column table;
 * + 64: the packer could NOT rule out that the reference's int32 running sum of some level wraps (exact_scalar.py:74-84,173-189) - the
 * exact formulation then differs from the reference on the inputs where the reference's own arithmetic wraps; TSIM_AMD_MODE=faithful
 * (every program) or =strict (exactly these programs) mirrors the wrap on the int32-faithful formulation */
int tsim_program_stats(const tsim_program *p, int64_t out[8]);

/* Which kernel family served the launches of this handle so far (diagnostics: scripts/shape_map.py, tests of the
 * eligibility rules - the reference takes every shape through one code path, src/tsim/sampler.py:117-167; here the shape
 * picks the kernel).  out[k] = launches of family k since creation / the last reset, TSIM_PATH_COUNT entries:
 * 0 k_sample_lw_fast (fused group), 1 k_sample_lw_fastm, 2 k_sample_lw_multi, 3 k_direct_multi, 4 k_sample_wide,
 * 5 k_sample_lw_fast (one batch), 6 k_sample_lw_reg, 7 k_sample_lw<false>, 8 k_sample_lw<true>, 9 k_sample4w,
 * 10 k_sample4, 11 k_sample4h, 12 k_sample_hw, 13 k_sample4_over, 14 row kernel (k_sample<W>), 15 k_sample4h_multi,
 * 16 k_sample_gen (fused group, any shape). */
#define TSIM_PATH_COUNT 24
int tsim_program_path_counts(tsim_program *p, int64_t out[TSIM_PATH_COUNT], int32_t reset);

const char *tsim_last_error(void);
const char *tsim_version(void);
/* The keys TSIM_AMD_TUNE="key=value,..." understands, comma separated (the launch planner's A/B switches; results never depend
 * on them - tests/test_gpu_knobs.py runs an oracle slice under every one).  No counterpart in the reference. */
const char *tsim_tune_keys(void);
/* The group schedule of tsim_sample_steps_device for the register first passes (host helper, no device): how many of the `left`
 * batches of B shots that remain in a call the next fused group takes.  fused_max: the cap (TSIM_AMD_TUNE fused_max, default 16);
 * long_shots: the fewest shots a group of more than 8 batches may hold (default 2^23, "fused_max=N:S" sets S).  Groups of more
 * than 8 only while at least 32 batches are left; everything else in even groups of at most 8.  No counterpart in the reference. */
int32_t tsim_steps_next_group(int32_t left, int64_t B, int32_t fused_max, int64_t long_shots);

#ifdef __cplusplus
}
#endif
#endif /* TSIM_HIP_H */

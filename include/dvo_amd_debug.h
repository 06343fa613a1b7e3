/*
 * dvo_amd_debug.h -- test probes, diagnostics and micro-benchmarks of libdvo_amd.so.
 *
 * NOT part of the drop-in boundary (that is dvo_amd.h: what a caller of dvo::DenseTracker / RgbdImagePyramid binds).  These
 * entry points exist for this repository's parity tests (stage probes, the receiving side of the record hand-off, band folds),
 * its bench (kernel timing, the isolated residual pass) and its profiling scripts (block trace, reducer stamps).  They are
 * exported by the same library, follow the same conventions (int status codes, nothing thrown) and may change without an ABI
 * version bump.
 */
#ifndef DVO_AMD_DEBUG_H_
#define DVO_AMD_DEBUG_H_

#include "dvo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (diagnostic; libraries built with -DDVO_TRACE_BLOCKS only, else -1) the per-block trace of every k_tick block since the last
 * call: 4 x 64-bit words per block {start, after the first step, end (100 MHz clock), info | hw_id << 32}; returns the number of
 * blocks recorded and resets the trace.  scripts/block_trace.py */
long long dvo_amd_debug_block_trace(dvo_amd_context *ctx, unsigned long long *out, long long capacity_blocks);
/* (test entry) out[i] = the table reciprocal of in[i] as the kernels compute it; needs DVO_AMD_RCP_HOST_SSE */
int dvo_amd_debug_rcp(dvo_amd_context *ctx, int n, const float *in, float *out);

/* host-only: the ordered combine of band records {valid, first_w, last_r0, last_r1, S[3], S_odd[3]} (10 doubles per band)
 * -> {valid, S[3], S_odd[3]}; exported for the CPU tests of the multi-GPU path */
int dvo_amd_debug_combine_bands(int n_bands, const double *bands, double *out);
/* host-only: the receiving side of the record hand-off.  A tick's 784-byte record reaches the host (and, for a sharded pair,
 * the peers) as `*n_pieces` pieces of 16 bytes -- two 8-byte halves {payload word, tick number} -- each written by one store
 * of the device; a piece counts when BOTH its tags are the tick waited for, in whatever order the pieces arrive (so a piece
 * that should ever arrive as two 8-byte halves is simply not accepted until both are there).
 * dvo_amd_debug_wire_layout reports the piece and payload-word counts; dvo_amd_debug_take_wire copies the payload of the
 * pieces from `from_piece` on that carry `tick` out of `wire` (16-byte aligned, 4 words per piece) into `record_words`
 * and returns the index of the first piece that does not (n_pieces when the record is complete), or minus an error code.
 * Exported for the CPU tests. */
/* host-only: the successor of a tick number (32 bits; never 0, the value of a fresh buffer; the wrap keeps the parity alternating) */
unsigned dvo_amd_debug_next_seq(unsigned seq);
int dvo_amd_debug_wire_layout(int *n_pieces, int *n_record_words);
int dvo_amd_debug_take_wire(const unsigned *wire, unsigned tick, int from_piece, unsigned *record_words);
/* host-only: where the blocks of one k_tick launch go (csrc/dvo_kernels.hip: tick_items_order, tick_args_layout and the host's
 * restatement of tick_locate), for a synthetic list of `n_items` (<= 62) work items.  Item i: res_blocks[i] residual blocks
 * of res_steps[i] steps per wave segment (one of the lengths a level can have: a power of two up to 64, or 6, 10, 12, 14, 18,
 * 20, 24, 30, 40) and ll_blocks[i] likelihood blocks; ref_key[i] / cur_key[i] name its reference level and its current level
 * (items with equal keys read the same arrays).  share: the value of DVO_AMD_SHARE_PLACEMENT (0, 1, 2); max_blocks: 0 = the
 * largest item's.  Out: order[k] = the item that goes k-th in the launch; per POSITION k of the launch group_first[k] (n_items +
 * 1 entries), xcd_rot[k], tail_rot[k], set_size[k]; *compact; *n_blocks = blocks of the one-dimensional grid; and, when the
 * grid is compact and block_item / block_index are given (capacity_blocks >= *n_blocks, else an error), for every block of
 * that grid the position of its item in the launch and which of the item's blocks it runs (-1, -1: a block that exits at once).
 * Exported for the CPU tests. */
int dvo_amd_debug_tick_layout(int n_items, const int *res_blocks, const int *ll_blocks, const int *res_steps, const int *ref_key,
                              const int *cur_key, int share, int max_blocks, int *order, int *group_first, int *xcd_rot,
                              int *tail_rot, int *set_size, int *compact, int *n_blocks, long long capacity_blocks, int *block_item,
                              int *block_index);

/* Stage-wise probe of ONE Gauss-Newton iteration body at a fixed pose (dense_tracking.cpp:271-347 without the accept test and
 * the solve): computeResidualsSse, computeWeightsSse (unit weights when precision_in is NULL = first iteration of a level,
 * else the t-distribution weights of the column-major 2x2 precision_in), computeScaleSse + inverse, the normal equations
 * (Mu = 0) and computeCompleteDataLogLikelihood, through exactly the kernels and host arithmetic dvo_amd_match uses (two
 * ticks).  Exists so that the parity tests can compare the weighted stages (iterations k >= 1) with their CPU checker directly
 * instead of only through the final pose. */
typedef struct {
  int valid_constraints;
  int reserved;
  double scale_sums[3];   /* unscaled pair sums (xx, xy, yy) of computeScaleSse incl. the Q5 pairing */
  float scale[4];         /* column-major 2x2: sums / (V - 3) */
  float precision[4];     /* its inverse (Eigen Matrix2f::inverse) */
  double moments[87];     /* the P-free sums (layout: dvo_types.h kAcc*) */
  double information[36]; /* A = sum w J^T P J, column-major 6x6 */
  double rhs[6];          /* b = -sum w J^T P r */
  double loglik_sum;      /* sum of log(1 + 0.2 r^T P r) over the first 50 floor(V/50) valid residuals (Q6) */
  float loglik;           /* what computeCompleteDataLogLikelihood returns */
  float reserved_f;
} dvo_amd_iteration_probe;
/* precision_eval (column-major 2x2, may be NULL): evaluate information / rhs / loglik with this precision instead of the one the
 * probe computed itself (out->precision is the computed one either way) */
int dvo_amd_debug_iteration(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level,
                            const float *T, const float *precision_in, const float *precision_eval,
                            dvo_amd_iteration_probe *out);

/* Host-rcpps mode only (dvo_amd_set_reciprocal_mode): the t-distribution weights of ONE residual pass at the float transform T
 * under the column-major 2x2 precision_in, as the product kernels form them -- the residual pass stores every pixel's weight
 * (weights[n pixels of the level], NaN where the pixel is no constraint) -- together with what k_q7_tail did about the pass's
 * last V mod 4 pixels (Q7, dense_tracking_impl.cpp:702-706: computeWeightsSse divides exactly there): which pixels, the weight
 * the pass gave them, computeWeight's, and what the difference adds to the pair sums and the 87 moments (k_finalize has added it
 * to the record by the time this returns).  The parity tests compare all of it with computeWeightsSse as this host runs it. */
typedef struct {
  int n_tail;             /* V mod 4 */
  int valid_constraints;  /* V of the record */
  int valid_counted;      /* V as k_q7_tail counted it from the block records */
  int recomputed_equal;   /* the tail pixels' recomputed residuals are the spilled ones, bit for bit */
  int pixel[3];           /* index in the level's scan order, ascending; -1 beyond n_tail */
  float weight_table[3];  /* 7 rcpps(5 + d) */
  float weight_exact[3];  /* (float)((2.0 + 5.0f) / (5.0f + d)) */
  double scale_sums_delta[3];
  double moments_delta[87];
} dvo_amd_q7_probe;
int dvo_amd_debug_weights(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level, const float *T,
                          const float *precision_in, float *weights, dvo_amd_q7_probe *tail);

/* (test entries) dvo_amd_residuals, dvo_amd_debug_iteration and dvo_amd_debug_weights over a MASKED selection: the points the pass
 * walks are those `mask` leaves of the selection of the context's thresholds, as for dvo_amd_match_masked (the same rules: the
 * mask's level-0 size and level count must fit the reference pyramid, DVO_AMD_ERR_INVALID_ARGUMENT / _DEVICE_MISMATCH otherwise; a
 * pyramid caches at most eight masked selections).  Everything else is the unmasked entry's body, shared, and a null mask IS the
 * unmasked entry.  They exist so that the parity tests can hold the order-dependent parts of the pass -- valid ranks carried across
 * wave segments, the Q5 parity stitch, the Q6 cut, the Q7 tail -- to their CPU checker on sparse selections, whose segments hold
 * few, one or no valid point (tests/test_sparse_passes.py). */
int dvo_amd_debug_residuals_masked(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level, const float *T,
                             const dvo_amd_mask *mask, float *residuals, int *n_valid);
int dvo_amd_debug_iteration_masked(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level,
                                   const float *T, const float *precision_in, const float *precision_eval,
                                   const dvo_amd_mask *mask, dvo_amd_iteration_probe *out);
int dvo_amd_debug_weights_masked(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level,
                                 const float *T, const float *precision_in, const dvo_amd_mask *mask, float *weights,
                                 dvo_amd_q7_probe *tail);

/* Diagnostic: the hardware queue the context's main stream runs on, asked of the GPU by a one-wave kernel on that stream (HW_ID:
 * pipe << 3 | queue).  The runtime maps streams onto its four hardware queues and a hardware queue runs one kernel at a time, so
 * how the trackers of a GPU are spread over them decides up to a third of a batch's throughput
 * (profiles/r05_stream_queue_assignment_ab.txt); the library takes the stream the runtime deals it (create the
 * trackers of a GPU back to back) and this entry lets an integrator look at the outcome.  Refused while pairs are queued. */
int dvo_amd_debug_hw_queue(dvo_amd_context *ctx, int *pipe_queue);

/* (test entry) the residual pass's geometry on one pyramid level under the context's configuration: `steps` 64-point steps per
 * wave segment -- what dvo_amd_config::segment_geometry documents (dvo_amd.h), a function of the level's size and the configuration
 * alone --, `points` the points the pass walks (the pixels the configuration's thresholds select, without an odd trailing one) and
 * `blocks` the blocks of four segments that cover them (tests/test_determinism.py pins the tables). */
int dvo_amd_debug_level_geometry(dvo_amd_context *ctx, dvo_amd_pyramid *reference, int level, int *steps, int *blocks, int *points);

/* Micro-benchmark of the dominant kernel alone (used by bench.py for the roofline figure and by the tuning scripts):
 * `reps` timed repetitions of the fused residual pass over `n_items` copies of one (reference level, current level) pair
 * at the float transform T (column-major 4x4), `rounds` 256-pixel rounds (four 64-pixel steps each) per wave segment (1, 2, 4, 8 or 16; 0 = the driver's choice).
 * avg_ms: HIP-event time per repetition on the context's stream; alg_bytes: 56 B x selected points x n_items;
 * n_launches: kernel launches one repetition needs (the argument block holds 62 items). */
int dvo_amd_bench_residual_pass(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level,
                                const float *T, int n_items, int rounds, int reps, double *avg_ms, double *alg_bytes,
                                int *n_launches);

/* the same over n_items DIFFERENT (reference, current) pairs (same size): no two items of a launch read the same planes, so
 * nothing is deduplicated by the caches */
int dvo_amd_bench_residual_pass_pairs(dvo_amd_context *ctx, int n_items, dvo_amd_pyramid *const *references,
                                      dvo_amd_pyramid *const *currents, int level, const float *T, int rounds, int reps,
                                      double *avg_ms, double *alg_bytes, int *n_launches);

/* Diagnostic: with DVO_AMD_FIN_STAMPS=1 in the environment the finalize kernel records 8 shader-clock stamps of its phases
 * (block 0 of the most recent launch); this reads them back. */
int dvo_amd_debug_finalize_stamps(dvo_amd_context *ctx, unsigned long long *stamps8);

/* Diagnostic: while dvo_amd_kernel_timing is enabled every k_tick launch is logged as 8 doubles {ms, items, residual-pass
 * blocks, likelihood blocks, grid.x, selected reference pixels of the residual items, 64-pixel wave steps of the residual
 * items, 64-pixel wave steps of the likelihood items}; this reads and clears the log (out may be NULL to query the count). */
int dvo_amd_debug_tick_log(dvo_amd_context *ctx, double *out, int capacity_records, int *n_records);

/* timing helper for bench.py: HIP-event milliseconds the context's stream spent in its residual-pass kernel since the last
 * reset, and the number of launches */
int dvo_amd_kernel_timing(dvo_amd_context *ctx, int enable, double *ms_residual_pass, long long *n_launches, int reset);

/* (diagnostic) which form of the host-rcpps mode the context's kernels run: 0 the mode is off, 1 a table in global memory (a gather
 * in the dependent chain of every step), 2 the device's own reciprocal of the cell midpoint plus 4-bit corrections from LDS (round
 * 5; bit-identical to form 1 by construction).  note: why form 2 is not in use ("" if it is or the mode is off). */
int dvo_amd_debug_rcp_form(const dvo_amd_context *ctx, int *form, char *note, int note_capacity);

/* (profiling aid) one no-op dispatch named `k_marker` on the context's main stream, waited for: bench.py brackets its
 * single-stream timing pass with two of them so that the summaries of a rocprofv3 run (kernel trace or counter pass) can select
 * exactly the k_tick dispatches in between (dvo_slam_amd/pmc.py) */
int dvo_amd_debug_marker(dvo_amd_context *ctx, unsigned tag);

/* (test entry) k_ll_overflow -- the exact answer to "did one of the reference's 50-term likelihood products overflow?"
 * (dense_tracking_impl.cpp:413-419) -- over a residual buffer the CALLER supplies, for one band of it: `residuals` = n_blocks x
 * 4 wave segments x (64 x steps) pixels x 2 floats in scan order, NaN = invalid pixel; the band = wave segments
 * [seg_first, seg_first + n_segs), rank_offset = valid pixels in earlier bands (the prefix table is built here from the NaN
 * pattern, relative to the band start, as k_finalize builds it); rank_end < 0: an open band (the walk may run on behind it);
 * rank_end >= 0: a CLOSED band of a pair sharded over several GPUs -- the residuals behind it are another rank's, whatever the
 * buffer holds there is stale and must not be looked at.  *overflowed = the kernel's verdict. */
int dvo_amd_debug_ll_overflow(dvo_amd_context *ctx, const float *residuals, int n_blocks, int steps, int seg_first, int n_segs,
                              int rank_offset, int rank_end, int cut_rank, const float *precision, int *overflowed);

/* the last dvo_amd_map_cloud / dvo_amd_voxel_downsample of the context: device time of its kernels from hipEvents inside the
 * call (input stage, sort, reduction; host gaps between them excluded), the time of the copy of the voxels to the host, and
 * the points it was handed.  scripts/map_cloud_timing.py */
int dvo_amd_debug_map_timing(dvo_amd_context *ctx, double *device_ms, double *copy_ms, long long *points);
/* the last dvo_amd_covisibility of the context (dvo_amd_find_constraint_candidates calls it too): device time of k_covis from
 * hipEvents inside the call.  scripts/covisibility_timing.py */
int dvo_amd_debug_covisibility_ms(const dvo_amd_context *ctx, double *device_ms);
/* the last dvo_amd_map_insert / _set_poses / _remove / _extract of a keyframe map: device time of its kernels from hipEvents
 * inside the call (host gaps excluded), the time of the copy of the voxels to the host (extract), the points and the voxels of
 * the delta it merged (0 for an extract), and the entries of one merge tile.  scripts/keyframe_map_timing.py */
int dvo_amd_debug_keyframe_map_timing(const dvo_amd_map *map, double *device_ms, double *copy_ms, long long *delta_points,
                                      long long *delta_voxels, int *merge_tile);
/* (test entry) the merge of a keyframe-map update on keys and sums the CALLER chooses: a store of na entries and a delta of nb
 * entries, host arrays, each side's keys ascending, distinct and below 2^63, the sums as eight 64-bit words per entry (count,
 * sx, sy, sz, r, g, b, pad).  The arrays are uploaded and merged by the launches of an update -- k_merge, the scan of its
 * flags, k_compact: the same kernels, none copied -- and the compacted store comes back: *n_out entries in keys_out / acc_out,
 * which hold na + nb entries each.  Sums of equal keys are added modulo 2^64; an entry whose count ends as 0 is dropped.  (An
 * update skips the merge when its delta is empty; this entry runs it whenever there is an entry at all.)
 * tests/test_voxel_edges.py */
int dvo_amd_debug_map_merge(dvo_amd_context *ctx, long long na, const unsigned long long *keys_a, const unsigned long long *acc_a,
                            long long nb, const unsigned long long *keys_b, const unsigned long long *acc_b,
                            unsigned long long *keys_out, unsigned long long *acc_out, long long *n_out);
/* the last dvo_amd_optimize_graph on the context: device ms of its first linearisation (linearise + assemble) and of its first
 * factorization (damped copy + blocked Cholesky), the padded system size, and the factorizations done */
int dvo_amd_debug_graph_timing(dvo_amd_context *ctx, double *linearise_ms, double *factorize_ms, int *n_padded,
                               int *factorizations);
/* the per-iteration records of graph `graph` of the last dvo_amd_optimize_graphs_batch on the context (the entry itself returns
 * only stats): at most `capacity` of them into `records`, *n_recorded = how many the call kept (the first 256 iterations) */
int dvo_amd_debug_graph_batch_records(dvo_amd_context *ctx, int graph, int capacity, dvo_amd_graph_iteration *records,
                                      int *n_recorded);
/* the first linear system of dvo_amd_optimize_graph on these inputs, before any step: H (n x n, row-major, full), b (n) and
 * F; x (n) = the undamped solve H x = b, valid when *failed_pivot < 0 (else the index of the first pivot <= 0).  Any of the
 * outputs may be NULL; H / b / x need 6 * (free active vertices) entries per side, *n_free says how many.  Poses are not moved. */
int dvo_amd_debug_graph_system(dvo_amd_context *ctx, int n_vertices, const double *poses, const int *fixed, int n_edges,
                               const dvo_amd_graph_edge *edges, double robust_delta, double *H, double *b, double *x,
                               double *F, int *n_free, int *failed_pivot);
/* the sparse counterpart of dvo_amd_debug_graph_system (options.solver = DVO_AMD_GRAPH_SOLVER_SPARSE): the stored 6 x 6 blocks
 * of H (*n_blocks of them, both mirror images, sorted by (row, col) slot; block_rc: row, col per block; blocks: 36 doubles
 * each, row-major), b and x (6 * n_free each, slot order; x = the undamped sparse solve, valid when *failed_pivot < 0, else
 * *failed_pivot >= 0 is an index within the failing front) and F.  More than block_capacity blocks: DVO_AMD_ERR_CAPACITY
 * with *n_blocks set.  Poses are not moved. */
int dvo_amd_debug_graph_system_sparse(dvo_amd_context *ctx, int n_vertices, const double *poses, const int *fixed,
                                      int n_edges, const dvo_amd_graph_edge *edges, double robust_delta, int block_capacity,
                                      int *n_blocks, int *block_rc, double *blocks, double *b, double *x, double *F,
                                      int *n_free, int *failed_pivot);
/* the sparse solver's symbolic phase on these vertices and edges (only from / to of an edge are read); needs no GPU.  Slots
 * are the free active vertices in increasing index.  perm (n_free): the slot eliminated k-th; per front (postorder, children
 * before parents): parent (-1 for a root), level (0 = leaves; a parent's level exceeds its children's), pivot slots and
 * update slots as CSR (pivot_ptr / update_ptr: n_fronts + 1 entries), both in elimination order; the predicted factor doubles
 * (nonzeros of L) and flops of one numeric factorization; the level count and the widest front (scalar dimension).  Every
 * array holds `capacity` ints; when n_free, n_fronts + 1 or n_update exceeds it the call returns DVO_AMD_ERR_CAPACITY with
 * the counts set.  Any output may be NULL. */
int dvo_amd_debug_graph_symbolic(int n_vertices, const int *fixed, int n_edges, const dvo_amd_graph_edge *edges,
                                 int capacity, int *n_free, int *n_fronts, int *n_update, int *n_levels, int *widest,
                                 int *perm, int *parent, int *level, int *pivot_ptr, int *pivot, int *update_ptr, int *update,
                                 double *factor_doubles, double *flops);
/* the last sparse dvo_amd_optimize_graph on the context: host ms of its symbolic phase; device ms (hipEvents) of its first
 * linearisation, of its first numeric factorization (assembly + partial factorization of every front) and of the
 * substitutions that follow it; the front count, level count, widest front (scalar dimension), predicted factor doubles and
 * flops */
int dvo_amd_debug_graph_sparse_timing(dvo_amd_context *ctx, double *symbolic_ms, double *linearise_ms, double *factorize_ms,
                                      double *solve_ms, int *fronts, int *levels, int *widest, double *factor_doubles,
                                      double *flops);
/* with enable != 0 every later pyramid build on `device` (any dvo_amd_pyramid_create* entry, the batched one as a whole) and
 * every later build of a point selection (the first dvo_amd_pyramid_select or match with a threshold pair; a selection found in
 * the pyramid's cache builds nothing and leaves the figure alone) is bracketed by two events on the device's internal stream;
 * *last_ms (may be NULL) receives the device time of the most recent bracketed build: uploads, ingest or remap, every level's
 * planes -- or a selection's kernels and its counter copy */
int dvo_amd_debug_ingest_timing(int device, int enable, double *last_ms);
/* what the most recent successful dvo_amd_pyramid_create_raw_batch on `device` enqueued: kernel launches (a function of the
 * level count and of build_selection alone, whatever the frame count), copies (two per host frame, the frame table, the
 * counters) and host synchronisations (one).  Any output may be NULL; all zero before the first such call */
int dvo_amd_debug_batch_build_stats(int device, int *kernel_launches, int *copies, int *synchronisations);
/* with enable != 0 every later dvo_amd_mask_combine, dvo_amd_mask_morph, dvo_amd_mask_warp and dvo_amd_mask_warp_many on `device`
 * is bracketed by two events on the device's internal stream, from before its first upload to behind its last kernel; *last_ms
 * (may be NULL) receives the device time of the most recent bracketed call */
int dvo_amd_debug_mask_ops_timing(int device, int enable, double *last_ms);
/* with enable != 0 the fusion launch of every later dvo_amd_pyramid_fuse_depth and dvo_amd_pyramid_fuse_depth_many on `device` is
 * bracketed by two events on the device's internal stream (the launch alone: not the tables' upload, not the pyramids' build);
 * *last_ms (may be NULL) receives the device time of the most recent bracketed launch */
int dvo_amd_debug_fuse_timing(int device, int enable, double *last_ms);
/* with enable != 0 the kernel launches of every later dvo_amd_place_scores, dvo_amd_place_query and dvo_amd_place_query_frames on
 * `device` are bracketed by two events on the device's internal stream, from before the first dot-product launch to behind the last
 * launch of the call (not the uploads, not a frame's descriptor, not the copies back); *last_ms (may be NULL) receives the device
 * time of the most recent bracketed call */
int dvo_amd_debug_place_timing(int device, int enable, double *last_ms);
/* what the most recent successful dvo_amd_pyramid_normals, dvo_amd_mask_from_normals or normal pass of
 * dvo_amd_point_cloud_normals on `device` enqueued: kernel launches (one, however many levels) and host synchronisations (one);
 * with enable != 0 the launch of every later such call is bracketed by two events on the device's internal stream (the launch
 * alone: not the table's upload, not the copies back) and *last_ms receives the device time of the most recent bracketed launch.
 * Any output may be NULL; all zero before the first such call */
int dvo_amd_debug_normals_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms);
/* with enable != 0 the filter launch of every later dvo_amd_pyramid_filter_depth and dvo_amd_pyramid_filter_depth_many on `device`
 * is bracketed by two events on the device's internal stream (the launch alone: not the tables' upload, not the pyramids' build);
 * *last_ms (may be NULL) receives the device time of the most recent bracketed launch */
int dvo_amd_debug_depth_filter_timing(int device, int enable, double *last_ms);
/* with enable != 0 every launch of a later dvo_amd_estimate_exposure / _many and dvo_amd_pyramid_adjust_intensity / _many on `device`
 * is bracketed by two events on the device's internal stream (the launches alone: not the tables' upload, not the host solve between
 * two passes, not the pyramids' build); *last_ms (may be NULL) receives the device time of the most recent bracketed call, its
 * launches added up */
int dvo_amd_debug_exposure_timing(int device, int enable, double *last_ms);
/* with enable != 0 every later dvo_amd_mask_filter_components, dvo_amd_mask_filter_components_many and dvo_amd_mask_components on
 * `device` is bracketed by two events on the device's internal stream, from before the upload of its plane table to behind its last
 * kernel (five launches for a filter, three for the inspection entry); *last_ms (may be NULL) receives the device time of the most
 * recent bracketed call */
int dvo_amd_debug_components_timing(int device, int enable, double *last_ms);
/* what the most recent successful dvo_amd_warp_inverse / _forward entry (plane or pyramid form, single or many) on `device`
 * enqueued of its own: kernel launches (1 for an inverse warp, 3 for a forward warp counting the clear, whatever n is) and host
 * synchronisations (one; a pyramid form's builder comes on top); with enable != 0 the launches of every later such call are
 * bracketed by two events on the device's internal stream (the launches alone: not the table's upload, not the copies back, not
 * the pyramids' build) and *last_ms receives the device time of the most recent bracketed call.  Any output may be NULL; all
 * zero before the first such call */
int dvo_amd_debug_warp_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms);
/* what the most recent successful dvo_amd_volume_integrate / _insert / _set_poses / _remove / _raycast / _raycast_pyramid / _extract
 * on `device` enqueued of its own: kernel launches (1 for an integration of any n and for a raycast, 3 for an extract: count, scan,
 * write; 2 when it ends at the capacity check) and host synchronisations (1; an extract: 2, the total comes back before the write);
 * a raycast pyramid's builder comes on top.  With enable != 0 the launches of every later such call are bracketed by two events on
 * the device's internal stream (the launches alone) and *last_ms receives the device time of the most recent bracketed call.  Any
 * output may be NULL; all zero before the first such call */
int dvo_amd_debug_volume_timing(int device, int enable, int *launches, int *synchronisations, double *last_ms);

#ifdef __cplusplus
}
#endif
#endif

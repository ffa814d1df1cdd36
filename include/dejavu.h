/*
 * dejavu.h -- C ABI of the MI355X scene-familiarity engine (libdejavu_hip.so).
 *
 * This is the drop-in boundary for the one hot path of navsim
 * (Linux-cpp-lisp/navigation-by-deja-vu): scoring sensor patches against the
 * stored-view library and picking the most familiar heading.  Plain C types
 * only; every host pointer is caller-owned and borrowed for the duration of the
 * call; outputs are caller-allocated; functions return DV_OK or a negative code
 * and never throw.  A context is single-threaded (one call in flight) and bound
 * to one GPU: multi-GPU runs use one process and one context per GPU.
 *
 * Reference interfaces replaced (citations into the reference repository):
 *   navsim/util.pyx:10-25        sads_familiarity(chem_weight)(scenes) -> func
 *   navsim/util.pyx:28-73        sads_hsv_metric(familiar_scenes, scene, fambuf, chem_weight)
 *   navsim/NavBySceneFamiliarity.py:283-316   heading loop of step_forward
 *   navsim/NavBySceneFamiliarity.py:140       library hand-off at train_from_path
 */
#ifndef DEJAVU_H
#define DEJAVU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dv_ctx dv_ctx;

enum {
    DV_OK = 0,
    DV_ERR_INVALID = -1,   /* bad argument (NULL, shape, chem_weight outside [0,1], A too large) */
    DV_ERR_HIP = -2,       /* a HIP runtime call failed; see dv_last_error */
    DV_ERR_STATE = -3,     /* no library set / no step to read back */
    DV_ERR_OOM = -4,       /* device or host allocation failed */
    DV_ERR_INDEX = -5      /* sensor footprint past the end of the landscape (the reference raises IndexError) */
};

#define DV_MAX_HEADINGS 64      /* headings scored per library pass */
#define DV_MAX_HUE_PLANES 4     /* distinct chemical hues handled by the one-hot layout */

/* dv_step flags */
#define DV_STEP_FORCE_RESOLVE 1u   /* run the exact tie resolver even for a single candidate */
#define DV_STEP_WANT_SCENE    2u   /* dv_step_enqueue: also produce scene_fam (dv_step: pass a buffer) */

/* dv_step_result.flags */
#define DV_RES_RESOLVED   1u       /* exact tie resolver ran; best_fam / exact_fam are bit-exact */
#define DV_RES_EXACT_ALL  2u       /* every score of this step is the exact sequential double */
#define DV_RES_OVERFLOW   4u       /* candidate list overflowed; step was redone in exact mode */
#define DV_RES_SENSE_ERROR 16u     /* batched calls: THIS agent's sensor footprint reached past the end of the landscape (the
                                      reference's IndexError for that trial); its other fields are meaningless.  The
                                      single-agent calls return DV_ERR_INDEX instead. */
#define DV_RES_RELOCALISED 32u     /* dv_rvreloc_*: THIS member's windowed familiarity lay below its threshold; its row is the
                                      whole-route step's, not the window's */

/*
 * Result of one step (replaces NavBySceneFamiliarity.py:313-316).
 * angle_fam[a]  = max over the (local) library of the familiarity of heading a
 *                 (:313); within 1e-12 relative of the reference's double, and
 *                 bit-exact for headings whose exact_fam is finite.
 * angle_view[a] = first view index (global = first_view + local) attaining it.
 * best_heading  = np.argmax(angle_familiarity) of the reference, bit-identical
 *                 (:315): near-ties are re-scored with the reference's exact
 *                 sequential double arithmetic before deciding.
 * exact_fam[a]  = exact max over the candidate views of heading a, -inf when
 *                 heading a has no candidate (only filled when RESOLVED).
 */
typedef struct dv_step_result {
    int32_t best_heading;
    uint32_t flags;
    int64_t best_view;
    double best_fam;
    double approx_max;          /* max over headings and views of the integer-sum score */
    double delta;               /* half-width of the candidate window around approx_max */
    int64_t n_candidates;       /* (heading, view) pairs inside the window */
    int32_t n_headings;
    int32_t reserved;
    double angle_fam[DV_MAX_HEADINGS];
    int64_t angle_view[DV_MAX_HEADINGS];
    double exact_fam[DV_MAX_HEADINGS];
    int64_t exact_view[DV_MAX_HEADINGS];
} dv_step_result;

typedef struct dv_lib_info {
    int64_t n_views;            /* F (local shard) */
    int64_t first_view;         /* global index of local view 0 */
    int32_t h, w;
    int32_t n_planes;           /* bytes stored per pixel on the device */
    int32_t n_hue_planes;       /* saturation planes stored (0 when chem_weight == 0) */
    int32_t generic_hue;        /* 1: more than DV_MAX_HUE_PLANES hues, H/S kept as planes */
    int32_t has_value_plane;    /* 0 when chem_weight == 1 */
    int64_t tile_bytes;         /* bytes the scoring kernel streams per pass */
    double chem_weight;
    double delta;               /* half-width of the candidate window around the best integer-sum score */
    uint8_t hues[DV_MAX_HUE_PLANES];
    int32_t n_hues;             /* distinct hues with S > 0 in the library (entries of hues[] that are valid) */
    int32_t signed_saturation;  /* 1: two hues, S <= 127: one plane holds 128 + S(hue0) - S(hue1) */
    /* bit-plane copy for the int8 matrix-core scoring path (libraries whose stored bytes come from few levels) */
    int32_t bit_planes_hs;      /* thermometer planes of the saturation bytes (0: no bit-plane copy, or none needed) */
    int32_t bit_planes_v;       /* thermometer planes of the value byte */
    int32_t has_bit_planes;     /* 1: the bit-plane copy exists (scoring shape 6 is available) */
    int32_t fp4_form;           /* 1: the planes also allow the fp4 form of that kernel (on-level patches, see dv_patches_on_level) */
    int64_t bit_tile_bytes;     /* bytes the matrix-core scoring kernel streams per pass (int8 form; fp4 form without code tiles) */
    int64_t code_tile_bytes;    /* bytes its fp4 form streams per pass when the value plane is stored as 3-bit level codes, else 0 */
    int32_t mixed_layout;       /* 1: the saturation planes take too many values for bit planes: the matrix-core kernel scores the
                                   value bit planes, a v_sad_u8 pass the saturation BYTE planes (bit_planes_hs is 0 and a step
                                   streams bit_tile_bytes + the saturation planes' share of tile_bytes) */
    int32_t reserved0;
    double weight_lo, weight_hi; /* chem_weights the layout serves for a weighted batch (dv_step_batch_weighted): [0, 1] when both
                                   sums are stored, [0, 0] without saturation planes, [1, 1] without the value plane */
} dv_lib_info;

/* ---- lifetime ---------------------------------------------------------- */
int dv_create(dv_ctx **out, int device_id);
void dv_destroy(dv_ctx *ctx);
/* Message of the last failure on ctx (or of the last failed dv_create when ctx is NULL). */
const char *dv_last_error(const dv_ctx *ctx);
/* Run on a caller-provided hipStream_t.  NULL restores the context's own stream, which is NON-BLOCKING: work on the
 * legacy null stream is not ordered with it, so pass a real stream to order this context with other work. */
int dv_set_stream(dv_ctx *ctx, void *hip_stream);
/* exact != 0: every score is the reference's sequential-double value (slower fp64 kernel). */
int dv_set_exact(dv_ctx *ctx, int exact);

/* ---- library (NavBySceneFamiliarity.py:122,140; util.pyx:10-13) ------- */
/*
 * views: uint8[F,h,w,3] C-contiguous, channels H,S,V.  Copied, re-tiled into
 * the device layout and released before return.  chem_weight must be in [0,1]
 * (util.pyx:12).  first_view is the global index of views[0] when the library
 * is sharded across GPUs (0 otherwise).
 */
int dv_set_library(dv_ctx *ctx, const uint8_t *views, int64_t n_views, int h, int w,
                   int channels, double chem_weight, int64_t first_view);
/*
 * Append n more views (uint8[n,h,w,3], same shape and chem_weight) to the resident library: a further training path
 * (scripts/run_experiment.py:23-26 anticipates several per library).  Existing views keep their device tiles, only the
 * new view groups are re-tiled; kernel forms timed on the library stay chosen.  The device layout was fixed by the
 * first ingest's hue set and saturation range: views outside it are refused with DV_ERR_STATE (re-ingest everything).
 */
int dv_append_library(dv_ctx *ctx, const uint8_t *views, int64_t n_views, int channels);
/* Same library as navsim_amd.synth.synth_views(seed, n_views, h, w, first_view), generated on the GPU. */
int dv_generate_library(dv_ctx *ctx, uint64_t seed, int64_t n_views, int h, int w,
                        double chem_weight, int64_t first_view);
/* The same with the saturation drawn from every value 0..127 (a swept concentration range, scripts/run_experiment.py:132,192)
 * when full_range_s != 0: such a library keeps its saturation planes as bytes (dv_lib_info.mixed_layout).  dv_generate_patches
 * then draws its patches' saturation the same way. */
int dv_generate_library_ex(dv_ctx *ctx, uint64_t seed, int64_t n_views, int h, int w, double chem_weight, int64_t first_view,
                           int full_range_s);
int dv_clear_library(dv_ctx *ctx);
int dv_get_library_info(const dv_ctx *ctx, dv_lib_info *out);
/*
 * The chem_weights later ingests (dv_set_library, dv_set_library_from_poses, dv_generate_library[_ex]) lay the library out for:
 * saturation planes are stored iff hi > 0, the value plane iff lo < 1, so that a weighted batch may give every agent a weight in
 * [lo, hi].  The ingest's own chem_weight must lie in the range (else the ingest fails with DV_ERR_INVALID); it stays the weight of
 * every unweighted step.  lo > hi (the default) restores the ingest's own weight alone.  dv_append_library* keep the layout
 * they find.
 */
int dv_set_weight_range(dv_ctx *ctx, double lo, double hi);
/*
 * Host arithmetic of the bit-plane layout (no context, no GPU): the thermometer planes of one stored byte plane from
 * the 256-bit presence map of its values (bit v of presence[v / 32] = value v occurs).  One plane per gap between
 * consecutive levels, gaps wider than 127 split, so that |a - b| = const(a) + sum_t bit_t(b) * (w[t] - 2 * clamp(a -
 * lo[t], 0, w[t])) with int8 coefficients for every byte a.  Returns the number of planes written to lo[] / w[]
 * (0 for a single level), -1 when more than `cap` would be needed.
 */
int dv_bitplane_plan(const uint32_t *presence, int cap, uint8_t *lo, uint8_t *w, int *lmin, int *lmax);
/*
 * Host arithmetic of the fp4 form of the matrix-core kernel for the n_planes planes dv_bitplane_plan gave one byte plane
 * (presence: the same 256-bit map): wfull[t] = the whole gap a plane stands for when it starts at a library level (its
 * int8 copies inside a gap wider than 127 get 0), wacc[bit] = the one width of the planes that land on bit `bit` of a
 * nibble (K-element n = plane n % n_planes sits on bit n % 4).  Returns 1 when every bit position has one width (the
 * exact fp4 coefficients +-1 exist for on-level patches), 0 when not, negative on bad arguments.
 */
int dv_fp4_plan(const uint32_t *presence, int n_planes, const uint8_t *lo, const uint8_t *w, uint8_t *wfull, int *wacc);
/* Copy the stored planes of local views [v0, v0+n) back as uint8[n, n_planes, h*w] (layout check). */
int dv_read_planes(dv_ctx *ctx, int64_t v0, int64_t n, uint8_t *out);

/* ---- sensor model (NavBySceneFamiliarity.py:151-192, util.pyx:91-168) -- */
/* landscape: uint8[rows, cols, 3] HSV, C-contiguous; copied to the GPU. */
int dv_set_landscape(dv_ctx *ctx, const uint8_t *landscape, int rows, int cols, int channels);
/*
 * sensor_dimensions = [sensor_w, sensor_h], sensor_pixel_dimensions = [pixel_w, pixel_h] (:90-96);
 * lut: uint8[3][256], the per-channel level quantisation of :176-186 tabulated by the caller;
 * mask_middle_n: columns zeroed either side of the middle (:189-190).
 */
int dv_configure_sensor(dv_ctx *ctx, int sensor_w, int sensor_h, int pixel_w, int pixel_h,
                        const uint8_t *lut, int mask_middle_n);
/* get_sensor_mat at n poses; out: uint8[n, sensor_h, sensor_w, 3].  DV_ERR_INDEX like the reference's IndexError. */
int dv_sense(dv_ctx *ctx, const double *x, const double *y, const double *angle, int n, uint8_t *out);
/* The A heading patches of one position straight into the resident patches (then dv_step_enqueue).  No host
 * synchronisation: a footprint past the end of the landscape is reported by the following dv_step_wait (DV_ERR_INDEX). */
int dv_sense_patches(dv_ctx *ctx, double x, double y, const double *angles, int n_headings);
/* One agent step's device work in one call: dv_sense_patches + dv_step_enqueue + dv_step_wait. */
int dv_sense_step(dv_ctx *ctx, double x, double y, const double *angles, int n_headings, uint32_t flags,
                  dv_step_result *result, double *scene_fam);
/*
 * Ensemble form: n_agents agents (positions x[i], y[i]; headings angles[i][0..A)) sensed and scored against the one
 * resident library, 64/A agents per library pass -- the trial farm of scripts/run_experiment.py:326-347 as agents
 * batched on one GPU.  results[n_agents].  An agent whose footprint leaves the landscape gets DV_RES_SENSE_ERROR in
 * its result's flags; the other agents' results are unaffected (the reference's trials are independent).
 */
int dv_sense_step_batch(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                        uint32_t flags, dv_step_result *results);
/*
 * dv_sense_step_batch with a chem_weight per agent: agent i is scored and decided under chem_weights[i] (the experiment grid's
 * chem_weight variable, scripts/run_experiment.py), all agents in the same library passes.  chem_weights == NULL is exactly
 * dv_sense_step_batch.  Refused (DV_ERR_INVALID) when a weight lies outside [0, 1], and (DV_ERR_STATE) when a weight needs a sum
 * the resident layout does not store (dv_lib_info.weight_lo / weight_hi; lay the library out with dv_set_weight_range first);
 * dv_last_error names the agent.
 */
int dv_sense_step_batch_weighted(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                                 const double *chem_weights, uint32_t flags, dv_step_result *results);
/*
 * dv_sense_step_batch_weighted that also returns every agent's scene_familiarity (NavBySceneFamiliarity.py:283-303 for each trial):
 * scene_fam = double[n_agents][F], non-NULL; scene_fam[i][f] = minimum over agent i's OWN n_headings headings of view f's familiarity
 * under chem_weights[i] (NULL: the library's weight) -- the values dv_sense_step(x[i], y[i], angles[i], ..., scene_fam) returns for
 * that pose on a library of that weight, bit for bit.  results as from dv_sense_step_batch_weighted (the same records).  An agent
 * with DV_RES_SENSE_ERROR gets a row of +inf (the reference has reset the array to inf before it senses, :287).  Argument errors as
 * for dv_sense_step_batch_weighted.  The passes keep their sums in HBM and run one after the other (as a single-agent step with
 * scene_fam does), so this is the call for reading the minimum, not for stepping; its row buffers are allocated at the first call
 * and grow only when a later call's passes hold more agents or views.  sads_hsv libraries only (DV_ERR_STATE otherwise).
 */
int dv_sense_step_batch_scene(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                              const double *chem_weights, uint32_t flags, dv_step_result *results, double *scene_fam);
/*
 * The device work AND the device-side book-keeping of one agent step in ONE call (the fast path of
 * navsim_amd.NavBySceneFamiliarity.step_forward; a 60 us step does not want three trips through a binding):
 *   1. when an error-metric answer is outstanding (dv_path_error_enqueue of an earlier step), it is collected:
 *      *have_nearest = 1, *nearest = the distance (update_error, NavBySceneFamiliarity.py:252-276); else *have_nearest = 0;
 *   2. when do_error != 0, the metrics of position (ex, ey) -- where the PREVIOUS step ended -- are asked for
 *      (dv_path_error_enqueue: on the context's second stream, beside this step's kernels);
 *   3. the headings (angle + offsets[a]) mod 2 pi (numpy's mod: the result takes the divisor's sign, :291) are sensed at
 *      (x, y) and scored as dv_sense_step does; angle_fam[n_headings] receives the per-heading maxima, *best_heading the
 *      decision (:313-315).  DV_ERR_INDEX like the reference's IndexError.
 */
int dv_agent_step(dv_ctx *ctx, double x, double y, double angle, const double *offsets, int n_headings,
                  int do_error, double ex, double ey, double reach,
                  double *angle_fam, int32_t *best_heading, double *nearest, int32_t *have_nearest);
/*
 * dv_agent_step in two halves: _begin does 1. and 2. and LAUNCHES 3. (returns at once), _end waits for the record and hands out
 * angle_fam / best_heading (and DV_ERR_INDEX).  The heading update between two steps (NavBySceneFamiliarity.py:317-323) serialises
 * them, but everything else the host does after a step -- book-keeping, stop tests, the caller's loop -- need not wait: an agent
 * begins its next step as soon as the new pose is known.  A begun step that is never ended is harmless (its record is not read);
 * any other step call in between makes _end fail with DV_ERR_STATE.
 */
int dv_agent_step_begin(dv_ctx *ctx, double x, double y, double angle, const double *offsets, int n_headings,
                        int do_error, double ex, double ey, double reach, double *nearest, int32_t *have_nearest);
int dv_agent_step_end(dv_ctx *ctx, double *angle_fam, int32_t *best_heading);
/*
 * _end and the next _begin in one call.  The caller has worked out, while the device was busy, where every candidate heading would
 * take the agent (cand_angle[a] = (angle + offsets[a]) mod 2 pi, cand_x / cand_y[a] = position + step_size (cos, sin), :317-321); the
 * call waits for the record and begins the next step at candidate *best_heading without returning in between -- unless that
 * position fails the reference's bounds test (:153-158; bounds = {r, cols - r, rows - r}), where the next step would stop before it
 * senses: *begun = 0.  do_error != 0 asks for the error metrics of the new position with the step begun (reach as in
 * dv_agent_step); nearest / have_nearest as in dv_agent_step_begin.
 */
int dv_agent_step_end_begin(dv_ctx *ctx, double *angle_fam, int32_t *best_heading, const double *cand_x, const double *cand_y,
                            const double *cand_angle, const double *offsets, int n_headings, const double *bounds, int do_error,
                            double reach, int32_t *begun, double *nearest, int32_t *have_nearest);
/* train_from_path (:118-140) on the device: sense n poses and ingest them as the library; out_views
 * (uint8[n, sensor_h, sensor_w, 3], may be NULL) receives familiar_scenes. */
int dv_set_library_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n,
                              double chem_weight, int64_t first_view, uint8_t *out_views);

/* dv_append_library with the views sensed on the device at n more poses (out_views may be NULL). */
int dv_append_library_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n,
                                 uint8_t *out_views);

/* ---- error / coverage metrics (NavBySceneFamiliarity.py:252-276) -------- */
/*
 * update_error of the reference on the device.  dv_set_training_path copies the training points (double[n][2], x then
 * y; NULL or n < 1 detaches) and clears the coverage marks.  dv_path_error_enqueue computes, for one agent position, the
 * distance to every training point in the reference's double arithmetic, marks the points within `reach`
 * (coverage_threshold_factor * step_size, :271) as covered, and leaves the smallest distance for
 * dv_path_error_wait, which returns the answers in the order they were asked for (at most 8 outstanding).  Nothing
 * here waits for the GPU except dv_path_error_wait / dv_path_coverage, so the metrics of step t are computed while
 * step t+1 is scored.  dv_path_coverage copies the marks back (uint8[n], 0/1); dv_path_reset clears them and drops
 * outstanding answers (reset_error, :195-203).
 */
int dv_set_training_path(dv_ctx *ctx, const double *xy, int64_t n);
int dv_path_error_enqueue(dv_ctx *ctx, double x, double y, double reach);
int dv_path_error_wait(dv_ctx *ctx, double *nearest);
int dv_path_coverage(dv_ctx *ctx, uint8_t *out, int64_t n);
int dv_path_reset(dv_ctx *ctx);
/*
 * The same metrics for the agents of an ensemble (navsim_amd.NavEnsemble; the reference farms its trials over MPI ranks, each with
 * its own update_error): dv_path_slots gives every agent a coverage array of its own on the device (n_slots x n_path bytes, cleared;
 * 0 frees them), dv_path_error_batch is update_error for n agents at once -- nearest[i] = agent i's distance to the nearest training
 * point in the reference's double arithmetic, its slot's marks updated -- synchronous (one kernel of n x ceil(n_path / 1024) blocks
 * per 64 agents).  dv_path_coverage_slot / dv_path_reset_slot (slot < 0: all) read / clear one agent's marks.
 */
int dv_path_slots(dv_ctx *ctx, int n_slots);
int dv_path_error_batch(dv_ctx *ctx, const int32_t *slots, const double *x, const double *y, int n, double reach, double *nearest);
int dv_path_coverage_slot(dv_ctx *ctx, int slot, uint8_t *out, int64_t n);
int dv_path_reset_slot(dv_ctx *ctx, int slot);
/*
 * The same metrics for an ensemble whose trials have training routes of their OWN (the reference's grid varies training_path_curve,
 * scripts/run_experiment.py:57,208).  These calls have buffers of their own: they leave the calls above and their results alone, and
 * the calls above leave them alone.
 *   dv_path_routes_set       xy = double[first[n_routes]][2], all routes' points, one route after the other; first = int64[n_routes + 1],
 *                            rising from first[0] = 0 (every route has at least one point).  NULL or n_routes = 0 detaches.  Drops the
 *                            slots and their marks.
 *   dv_path_routes_slots     slot j gets coverage marks of its own for route route_of_slot[j]: exactly that route's length in bytes,
 *                            cleared; the arrays lie back to back without padding.  n_slots = 0 frees them.
 *   dv_path_routes_error     update_error for n entries at once: entry i is slot slots[i] standing at (x[i], y[i]) with its OWN
 *                            reach[i].  nearest[i] = the distance to the nearest point of that slot's route, in the reference's
 *                            double arithmetic; the slot's marks get `dist <= reach[i]` OR-ed in.  Entries are independent, and a
 *                            slot may occur more than once.  Synchronous: one upload of the entry table, one kernel launch per
 *                            65 535 entries, one copy back and one wait, whatever n is.
 *   dv_path_routes_coverage  copies slot's marks out (uint8[n], 0/1); n must be the length of the slot's route.
 *   dv_path_routes_reset     clears one slot's marks, or all with slot < 0.
 *   dv_path_routes_info      the counts: routes, slots, points of all routes (any pointer may be NULL).
 * Every route_of_slot and slots entry is checked before anything is enqueued: DV_ERR_INVALID names the first bad one, and nothing
 * is marked or reallocated.  Without routes (or, for error / coverage / reset, without slots): DV_ERR_STATE.  On DV_ERR_OOM routes,
 * slots and marks stay as they were.
 */
int dv_path_routes_set(dv_ctx *ctx, const double *xy, const int64_t *first, int n_routes);
int dv_path_routes_slots(dv_ctx *ctx, const int32_t *route_of_slot, int n_slots);
int dv_path_routes_error(dv_ctx *ctx, const int32_t *slots, const double *x, const double *y, const double *reach, int64_t n,
                         double *nearest);
int dv_path_routes_coverage(dv_ctx *ctx, int slot, uint8_t *out, int64_t n);
int dv_path_routes_reset(dv_ctx *ctx, int slot);
int dv_path_routes_info(dv_ctx *ctx, int *n_routes, int *n_slots, int64_t *n_points);
/*
 * The three coverage statistics of a trial's result row (percent_recapitulated, percent_recapitulated_forgiving, n_captures;
 * NavBySceneFamiliarity.py:212-249) taken from the marks where they lie, instead of copying the marks out and looping over them on
 * the host.  With n marks, run[p] the number of consecutive set marks ending at p (0 where mark p is clear) and `window` the number
 * of marks the reference takes as int(n_consecutive_scenes * n), an entry's three int64 are
 *     covered  = the number of set marks                                     (path coverage = covered / n)
 *     furthest = the largest p + 1 with run[p] >= window, 0 without one      (forgiving coverage = furthest / n)
 *     captures = the number of p in [window, n) with run[p] == window        (n_captures)
 * which equal the reference's loops for every window >= 0 (window = 0: furthest = n, captures = the clear marks; window > n: both 0).
 *   dv_marks_summary         the agent's marks (those dv_path_coverage copies out): out3 = int64[3].
 *   dv_marks_summary_slots   n entries over the slots of dv_path_slots: entry i is slot slots[i] under window[i]; out = int64[n][3].
 *   dv_marks_summary_routes  the same over the slots of dv_path_routes_slots, each as long as its own route.
 * Entries are independent, and a slot may occur more than once with different windows.  The calls only read marks.  They run on the
 * context's stream behind every metrics call made before them, and are synchronous: one upload of the entry table, one kernel launch
 * per 65 535 entries (a workgroup per entry, DV_MARKS_PER_TRIP marks a trip, DV_MARKS_PER_THREAD per thread), one copy back and one
 * wait.  Every slot and every window is checked before anything is enqueued: DV_ERR_INVALID names the first entry out of range or
 * below 0.  Without a training path, slots or routes: DV_ERR_STATE.  n = 0: DV_OK, nothing happens.  Marks and index arithmetic are
 * 64-bit: no length is refused.
 */
#define DV_MARKS_PER_THREAD 16
#define DV_MARKS_PER_TRIP 4096
int dv_marks_summary(dv_ctx *ctx, int64_t window, int64_t *out3);
int dv_marks_summary_slots(dv_ctx *ctx, const int32_t *slots, const int64_t *window, int n, int64_t *out);
int dv_marks_summary_routes(dv_ctx *ctx, const int32_t *slots, const int64_t *window, int64_t n, int64_t *out);

/* ---- scoring ----------------------------------------------------------- */
/* func(scene, fambuf) of util.pyx:14-20: fambuf[f] for one patch uint8[h,w,3] against every local view. */
int dv_score(dv_ctx *ctx, const uint8_t *patch, double *fambuf);
/*
 * One navigation step's scoring (NavBySceneFamiliarity.py:283-316) for
 * patches uint8[A,h,w,3], A <= DV_MAX_HEADINGS.
 * scene_fam: double[F] or NULL -- min over headings per view (:301-303).
 */
int dv_step(dv_ctx *ctx, const uint8_t *patches, int n_headings, uint32_t flags,
            dv_step_result *result, double *scene_fam);
/*
 * Ensemble form: n_agents agents, each with its own n_headings patches (uint8[n_agents, A, h, w, 3]), against
 * the same library; results[n_agents].  Agents are scored DV_MAX_HEADINGS / A at a time in one library pass.
 */
int dv_step_batch(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, uint32_t flags,
                  dv_step_result *results);
/* dv_step_batch with a chem_weight per agent; the rules of dv_sense_step_batch_weighted. */
int dv_step_batch_weighted(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const double *chem_weights,
                           uint32_t flags, dv_step_result *results);
/* dv_step_batch_weighted that also returns scene_fam = double[n_agents][F]; the rules of dv_sense_step_batch_scene. */
int dv_step_batch_scene(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const double *chem_weights,
                        uint32_t flags, dv_step_result *results, double *scene_fam);
/* Re-run the exact resolver on the candidates of the last step (sharded runs, cross-rank ties). */
int dv_resolve(dv_ctx *ctx, dv_step_result *result);

/* ---- steps of ANY number of headings ------------------------------------ */
/*
 * The reference takes any n_test_angles (NavBySceneFamiliarity.py:62,87-88; its loop :289 runs over all of them, its default
 * is 60); dv_step / dv_sense_step hold at most DV_MAX_HEADINGS because their result record is a fixed structure.  The wide
 * forms take 1 <= n_headings <= DV_MAX_WIDE_HEADINGS: the headings are scored DV_MAX_HEADINGS per library pass (the passes
 * enqueued back to back, their records collected afterwards) and the passes' decisions merged on the host by the rule of
 * NavBySceneFamiliarity.py:313-315 -- the first heading attaining the maximum; where two passes' maxima lie within the
 * candidate window of each other the passes concerned are re-scored by the exact resolver first and the exact values
 * compared, so best_heading is bit-identical to np.argmax of the reference for any n_headings.
 * angle_fam[n_headings] (caller-allocated) receives every heading's maximum, angle_view[n_headings] (may be NULL) its first
 * view, scene_fam[F] (may be NULL) the minimum over ALL headings per view (:301-303).
 */
#define DV_MAX_WIDE_HEADINGS 4096
typedef struct dv_wide_result {
    int32_t best_heading;       /* index into the n_headings headings */
    uint32_t flags;             /* DV_RES_* of the pass that won */
    int64_t best_view;
    double best_fam;
    int32_t n_headings;
    int32_t n_passes;           /* library passes this step took (re-scored passes not counted) */
    int32_t n_contending;       /* passes whose maximum lay within the candidate window of the overall one */
    int32_t reserved;
} dv_wide_result;
int dv_step_wide(dv_ctx *ctx, const uint8_t *patches, int n_headings, uint32_t flags, dv_wide_result *result,
                 double *angle_fam, int64_t *angle_view, double *scene_fam);
int dv_sense_step_wide(dv_ctx *ctx, double x, double y, const double *angles, int n_headings, uint32_t flags,
                       dv_wide_result *result, double *angle_fam, int64_t *angle_view, double *scene_fam);

/* ---- ssd_f32 metric (the reference's `ssds`, navsim/util.pyx:171-184) ---- */
/*
 * views: float32[F,h,w] single channel.  Scores are sums of squared differences (smaller = more familiar):
 * fp32 fma over 16 pixels folded into a double, within ~1e-6 relative of ssds() on the upcast data; the chosen
 * heading / view are those of the exact double sums (near-ties within 3e-6 relative are re-scored exactly).
 * Up to DV_MAX_HEADINGS headings per step, scored 16 per pass over the library.  In the result, angle_fam[a] = min over views of the SSD of heading a,
 * best_heading = first heading attaining the overall minimum; scene_ssd[f] = max over headings.
 */
int dv_set_library_f32(dv_ctx *ctx, const float *views, int64_t n_views, int h, int w, int64_t first_view);
/* Same library as navsim_amd.synth.synth_views_f32(seed, n_views, h, w, first_view), generated on the GPU (BASELINE.json
 * configs[2] in its literal form is 500 000 x 128x128 float32 = 32.8 GB: made where it is scored, not uploaded). */
int dv_generate_library_f32(dv_ctx *ctx, uint64_t seed, int64_t n_views, int h, int w, int64_t first_view);
int dv_score_f32(dv_ctx *ctx, const float *patch, double *ssdbuf);
int dv_step_f32(dv_ctx *ctx, const float *patches, int n_headings, uint32_t flags, dv_step_result *result,
                double *scene_ssd);

/* ---- ssd_u8 metric (the same `ssds`, navsim/util.pyx:171-184, for uint8 views) ---- */
/*
 * views: uint8[F,h,w] single channel, h * w <= 131071.  Scores are the EXACT integer sums of squared differences -- what ssds()
 * returns for the same data as float64 -- computed on the int8 matrix cores (sum (a-b)^2 = sum a'^2 + sum b'^2 - 2 sum a'b' with
 * a' = a - 128).  Ties go to the first heading, then the first view; nothing is re-scored.  Up to DV_MAX_HEADINGS headings per step,
 * 32 per pass over the library (one byte per pixel).  Results as dv_step_f32's.
 */
int dv_set_library_u8(dv_ctx *ctx, const uint8_t *views, int64_t n_views, int h, int w, int64_t first_view);
int dv_score_u8(dv_ctx *ctx, const uint8_t *patch, double *ssdbuf);
int dv_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_headings, uint32_t flags, dv_step_result *result,
               double *scene_ssd);
/*
 * The ssd_u8 metric behind the sensor model: what the agent's step needs when SSD is its familiarity plug-in
 * (navsim_amd.util.ssd_familiarity).  `channel` (0 H, 1 S, 2 V) picks the byte of each sensed HSV pixel that is compared.
 * dv_set_library_u8_from_poses = train_from_path (NavBySceneFamiliarity.py:118-140) on the device: senses n poses, hands back
 * familiar_scenes (out_views: uint8[n, sensor_h, sensor_w, 3], may be NULL) and ingests the chosen channel as the ssd_u8 library.
 * dv_sense_step_u8 = dv_sense_step for that library: the A heading patches are sensed at (x, y), their channel scored on the
 * int8 matrix cores, the least-SSD heading decided on the device; DV_ERR_INDEX like the reference's IndexError.
 */
int dv_set_library_u8_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n, int channel,
                                 int64_t first_view, uint8_t *out_views);
int dv_sense_step_u8(dv_ctx *ctx, double x, double y, const double *angles, int n_headings, int channel, uint32_t flags,
                     dv_step_result *result, double *scene_ssd);

/* ---- resident / asynchronous form (benchmarks, pipelined callers) ------ */
/* Upload patches and prepare their device layout; no host synchronisation. */
int dv_upload_patches(dv_ctx *ctx, const uint8_t *patches, int n_headings);
/* Generate patches on the device: synth_views(seed + 1, n_headings, h, w). */
int dv_generate_patches(dv_ctx *ctx, uint64_t seed, int n_headings);
/* Enqueue one step on the resident patches (scoring, reductions, tie resolver); no host synchronisation. */
int dv_step_enqueue(dv_ctx *ctx, uint32_t flags);
/* Wait for the last enqueued step and copy its result (and optionally scene_fam[F]). */
int dv_step_wait(dv_ctx *ctx, dv_step_result *result, double *scene_fam);
/*
 * Device address of the packed record of the last enqueued step, for a device-side exchange between ranks
 * (stream-ordered after dv_step_enqueue on the context's stream; no host synchronisation):
 *   double[3 + 4A] = approx_max, n_candidates, state (0 integer scores, 1 candidates exact, 2 all exact; + 4 when the
 *                    patches were sensed past the end of the landscape: dv_merge_records then returns DV_ERR_INDEX),
 *                    angle_fam[A], angle_view[A], exact_fam[A], exact_view[A]
 */
int dv_step_record(dv_ctx *ctx, void **device_ptr, int *n_doubles);
/*
 * The sharded step's fast exchange: packed keys of the last enqueued step for ONE all-reduce(max) of uint64 words
 * (north star: one all-reduce per navigation step).  dv_step_keys enqueues, behind the step, the kernel that builds
 *   keys[a], a < A              ordered image of this rank's max over its views of heading a's score
 *   keys[A + 4r .. A + 4r + 3]  rank r's slot (zero on the other ranks): ordered image of its best score; candidate
 *                               count | state << 32 | 1 << 48; its first-maximum heading + 1; that heading's view + 1
 * and returns their device address (n_words = A + 4 * world).  signed_order != 0 flips every word's top bit, so that a
 * signed 64-bit maximum orders them correctly.  dv_merge_keys (host arithmetic only, no context) takes the reduced
 * words: when a single (heading, view) pair lies within delta of the global maximum it fills the decision, else it
 * sets needs_resolve and the full records are exchanged (dv_step_record / dv_merge_records).  DV_ERR_INDEX when a rank
 * reports patches sensed past the end of the landscape.
 */
int dv_step_keys(dv_ctx *ctx, int rank, int world, int signed_order, void **device_ptr, int *n_words);
/* Enqueue the exact resolver on the last step's candidates (updates the record); no host synchronisation. */
int dv_resolve_enqueue(dv_ctx *ctx);
/*
 * Hand a device buffer (e.g. the output of an all-gather of the ranks' records) to the host without a blocking
 * stream synchronisation: dv_publish enqueues, on the context's stream, a copy of n_doubles doubles into mapped host
 * memory followed by a sequence word; dv_publish_wait polls that word and copies the doubles to dst.
 */
int dv_publish(dv_ctx *ctx, const void *device_src, int64_t n_doubles);
int dv_publish_wait(dv_ctx *ctx, double *dst, int64_t n_doubles);

/*
 * Mailbox exchange for the ranks of ONE node (an alternative to an all-gather: no collective kernel at all).
 * host_base: a page-aligned host segment that every rank's process has mapped (e.g. a file in /dev/shm), laid out as
 * [slots][world][512 doubles]; dv_set_mailbox registers it with this context's GPU (NULL detaches).
 * dv_mailbox_post enqueues, behind the step's kernels, the copy of this rank's packed record (dv_step_record) into
 * entry [slot][rank] with sequence number seq; dv_mailbox_wait polls (host) until the ranks of rank_mask have posted
 * seq into `slot` and copies their records to records[r * stride ..] (timeout_ms <= 0: wait for ever).  A slot may be
 * reused once every rank has read it: two slots per exchange round alternate safely, because nobody posts step
 * s + 2 before everybody has posted step s + 1, i.e. has finished reading step s.
 */
int dv_set_mailbox(dv_ctx *ctx, void *host_base, int64_t bytes, int rank, int world);
int dv_mailbox_post(dv_ctx *ctx, int slot, uint64_t seq);
int dv_mailbox_wait(dv_ctx *ctx, int slot, uint64_t seq, uint64_t rank_mask, double *records, int64_t stride, int timeout_ms);

/*
 * The global decision from the gathered per-rank records (the sharded form of NavBySceneFamiliarity.py:313-316);
 * identical on every rank.  records[r * stride .. ] is rank r's record as laid out by dv_step_record.  Host
 * arithmetic only: no context, no GPU.  When ranks that contend for the maximum (approx_max within delta of the
 * global one) hold more than one candidate pair between them and one of them has not re-scored its candidates yet,
 * needs_resolve is set and no decision is made: those ranks (contending_mask, bit r = rank r, world <= 64) run
 * dv_resolve_enqueue and the records are exchanged again.
 */
typedef struct dv_merge_out {
    int32_t best_heading;
    int32_t resolved;           /* 1: exact values decided; 0: a single candidate pair, integer scores decided */
    int64_t best_view;
    double best_fam;
    int32_t needs_resolve;
    int32_t n_contending;
    uint64_t contending_mask;
    double angle_fam[DV_MAX_HEADINGS];
} dv_merge_out;
int dv_merge_records(const double *records, int world, int n_headings, int64_t stride, double delta, dv_merge_out *out);
int dv_merge_keys(const uint64_t *keys, int world, int n_headings, double delta, int signed_order, dv_merge_out *out);
int dv_synchronize(dv_ctx *ctx);

/* ---- one process, several devices ---------------------------------------- */
/*
 * SURVEY 8-b2 words the boundary as dv_create(ctx**, device_ids[], n): one caller thread that owns all GPUs of a node (the
 * reference is a single Python process, navsim/NavBySceneFamiliarity.py:72,140,299).  A dv_group is that form: n contexts, member r
 * on device_ids[r], behind one handle.  The library is cut into contiguous blocks of views in member order (first members take
 * the extras), every member's step is enqueued before any is waited for, and the members' records are merged by the sharded
 * step's rules (dv_merge_records; near-ties across members are re-scored exactly by the contending members, dv_resolve) -- the
 * decision is the unsharded one, first occurrence included (:313-315).  The multi-PROCESS form (one rank per GPU, one RCCL
 * all-reduce per step) is navsim_amd/sharded.py over dv_step_keys / dv_step_record.
 *   dv_group_step        patches uint8[A, h, w, 3] go to every member; scene_fam (may be NULL) receives float64[F] in library order
 *   dv_group_sense_step  every member senses the patches from its own copy of the landscape (dv_group_set_landscape,
 *                        dv_group_configure_sensor): nothing but the pose goes up
 *   dv_group_score       func(scene, fambuf) of the plug-in (util.pyx:14-20): fambuf[F]
 *   result               best_heading / best_view (global index) / best_fam, angle_fam[A] and angle_view[A] (maxima over all
 *                        members and their first views), flags DV_RES_RESOLVED when exact values decided; exact_* unused
 * The same device id may be given more than once (independent contexts on one GPU).
 */
typedef struct dv_group dv_group;
int dv_group_create(dv_group **out, const int *device_ids, int n_devices);
void dv_group_destroy(dv_group *g);
const char *dv_group_last_error(const dv_group *g);
int dv_group_size(const dv_group *g);
int dv_group_member(dv_group *g, int r, dv_ctx **ctx, int64_t *first_view, int64_t *n_views);
int dv_group_set_library(dv_group *g, const uint8_t *views, int64_t n_views, int h, int w, int channels, double chem_weight);
int dv_group_set_landscape(dv_group *g, const uint8_t *landscape, int rows, int cols, int channels);
int dv_group_configure_sensor(dv_group *g, int sensor_w, int sensor_h, int pixel_w, int pixel_h, const uint8_t *level_lut,
                              int mask_middle_n);
int dv_group_score(dv_group *g, const uint8_t *patch, double *fambuf);
int dv_group_step(dv_group *g, const uint8_t *patches, int n_headings, uint32_t flags, dv_step_result *result, double *scene_fam);
int dv_group_sense_step(dv_group *g, double x, double y, const double *angles, int n_headings, uint32_t flags,
                        dv_step_result *result, double *scene_fam);

/* ---- landscape generator: the 2-D heat equation ---------------------------- */
/*
 * diffuse of the reference (navsim/util.pyx:189-235): the explicit five-point scheme under periodic boundaries on a square
 * float64 field, `nstep` full sweeps, every cell
 *     new = m + multiplier * ((((m[i+1,j] + m[i-1,j]) - 4*m[i,j]) + m[i,j+1]) + m[i,j-1])
 * with multiplier = c * (delta_t / (delta_s * delta_s)), delta_s = 1 / (n + 1), delta_t = delta_t_factor * (delta_s^2 / (2c)),
 * each operation rounded on its own (no fused multiply-add), so the field carries the reference's bits after every step.
 * The field lives in two device buffers of the context, on its device and stream, beside (and independent of) a resident
 * library, landscape, patches and training path.  The reference's sanity checks (sum, maximum, minimum, NaN) are the
 * caller's: navsim_amd/generate_landscapes.py runs them in NumPy as the reference does.
 *   begin     uploads float64[n, n] and fixes the multiplier; DV_ERR_INVALID for n < 1, c == 0 or a NULL field.  A field
 *             already there is replaced.
 *   advance   nstep >= 0 more steps, enqueued.  DV_DIFFUSE_PLAIN: one launch per step between the two buffers.
 *             DV_DIFFUSE_BLOCKED: a workgroup advances a tile plus its halo `steps_per_launch` steps in LDS per launch (the
 *             rest of nstep in a shorter launch).  DV_DIFFUSE_AUTO: whichever was measured faster.  All give the same bits.
 *   read      the current field into float64[n, n]; waits for the stream.
 *   end       frees the buffers.
 *   configure window side (64 or 96) and steps per launch (1..44, cut to what the window allows) of the blocked form for later
 *             advances, for A/B; 0 keeps a value.  Defaults: DEJAVU_DIFFUSE_S / DEJAVU_DIFFUSE_T at dv_create, else 64 and 8.
 *   info      tile side and steps per launch of the blocked form, and the steps advanced since begin (0 without a field);
 *             any pointer may be NULL.
 * advance / read without a field: DV_ERR_STATE.  The last declaration is the one-shot call made of the others.
 */
#define DV_DIFFUSE_AUTO    0u
#define DV_DIFFUSE_PLAIN   1u
#define DV_DIFFUSE_BLOCKED 2u
int dv_diffuse_begin(dv_ctx *ctx, const double *init, int n, double c, double delta_t_factor);
int dv_diffuse_advance(dv_ctx *ctx, int64_t nstep, uint32_t flags);
int dv_diffuse_read(dv_ctx *ctx, double *out);
int dv_diffuse_end(dv_ctx *ctx);
int dv_diffuse_configure(dv_ctx *ctx, int window, int steps_per_launch);
int dv_diffuse_info(dv_ctx *ctx, int *tile, int *steps_per_launch, int *steps_done);
int dv_diffuse(dv_ctx *ctx, const double *init, int n, int64_t nstep, double c, double delta_t_factor, uint32_t flags, double *out);

/* ---- Infomax familiarity model -------------------------------------------- */
/*
 * A second familiarity model behind the reference's plug-in seam (navsim/util.pyx:10-25): the Infomax network of Baddeley, Graham,
 * Husbands & Philippides (2012).  One layer of weights W, float64[M, N], N = h * w sensor pixels, M = n_hidden, trained in one pass
 * over the route's views; memory and the cost of a step do not grow with the route.  With p the view's compared plane (uint8[h, w],
 * C order) and x = p/255 - mean(p/255) in float64, a training view does
 *     h = W x;  y = tanh(h);  u = h^T W;  W <- W + (learning_rate / N) * (W - (y + h) u^T)
 * and a scored view has unfamiliarity d(x) = sum_i |(W x)_i|; the calls report familiarity = -d (so the reference's np.max /
 * np.argmax pick the least novel heading; the largest possible value is 0).  Everything is float64 on the device, no reduction
 * uses floating-point atomics and each has a fixed order: the same calls on the same bytes give the same bits.  The model lives
 * beside, and independent of, a resident library, landscape, patches and diffuse field.
 *   begin            allocates W and copies w0 (float64[n_hidden * h * w], row-major; the caller draws it).  A model already there
 *                    is replaced.  DV_ERR_INVALID: channel outside {0, 1, 2}, learning_rate <= 0, n_hidden < 1, h or w < 1, NULL w0.
 *                    DV_ERR_OOM when W does not fit.
 *   train_u8         trains on uint8[n, h, w] planes in order; calling it again continues the chain (train(a) then train(b) gives
 *                    the bits of train(a + b)).
 *   train_from_poses senses the n poses as dv_set_library_from_poses does and trains on their `channel` plane with no host round
 *                    trip; out_views (may be NULL) receives uint8[n, h, w, 3].  DV_ERR_INDEX as dv_sense; DV_ERR_INVALID when the
 *                    sensor's shape is not the model's.
 *                    Both: after training, one reduction checks that W is finite; if not (a too-large learning rate makes the rule
 *                    diverge) the call returns DV_ERR_STATE, dv_last_error names the learning rate, and training and scoring keep
 *                    returning DV_ERR_STATE until begin or set_weights brings finite weights.
 *   score_u8         familiarity[a] = -d of each of uint8[n, h, w] planes, any n >= 1 (64 per pass over W).
 *   sense_step       one agent step: senses the n_headings patches at (x, y), scores their `channel` plane and takes the first
 *                    maximum of angle_fam (np.argmax).  Any n_headings >= 1.  DV_ERR_INDEX like dv_sense_step.
 *   dv_batch_infomax_step_u8 / dv_batch_infomax_sense_step   an ensemble's step.  (The dv_infomax_ prefix is kept to the single
 *                    model's nine calls; the ensemble's two are named apart from it.)  n_agents members of n_headings headings
 *                    each share the one W, their n_agents * n_headings patches being columns of one H = W X (member i owns
 *                    columns [i * n_headings, (i + 1) * n_headings)).  batch_infomax_step_u8 scores uploaded planes
 *                    uint8[n_agents][n_headings][h][w]; batch_infomax_sense_step senses member i at (x[i], y[i]) along
 *                    angles[i][0 .. n_headings).  angle_fam[n_agents][n_headings] and best_heading[n_agents] (each member's first
 *                    maximum, np.argmax) come back from ONE enqueue and ONE wait, whatever n_agents is; the sums, the negation
 *                    and the maxima are taken on the device.  Any n_agents >= 1 and n_headings >= 1 (also > 64).  A column's
 *                    value has the bits score_u8 / sense_step give the same patch.  batch_infomax_sense_step does not fail for
 *                    a footprint that leaves the landscape: flags[i] (uint32[n_agents]) carries DV_RES_SENSE_ERROR for such a
 *                    member, its best_heading is -1 and its row of angle_fam unspecified; the other members' results are
 *                    untouched (as dv_sense_step_batch).  State, sensor-shape and non-finite-weight errors as sense_step;
 *                    DV_ERR_INVALID for a NULL pointer, n_agents < 1 or n_headings < 1.
 *   read_weights / set_weights   copy float64[n_hidden * h * w] out and in: what a user saves and restores.
 *   info             n_hidden, n_pixels, views trained since begin, whether W is finite (0 without a model), bytes of W; any
 *                    pointer may be NULL.
 *   end              frees the model; dv_destroy frees it too.
 * Every call but begin, info and end returns DV_ERR_STATE without a model.
 */
int dv_infomax_begin(dv_ctx *ctx, int h, int w, int channel, int n_hidden, double learning_rate, const double *w0);
int dv_infomax_train_u8(dv_ctx *ctx, const uint8_t *planes, int64_t n);
int dv_infomax_train_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n, uint8_t *out_views);
int dv_infomax_score_u8(dv_ctx *ctx, const uint8_t *planes, int n, double *familiarity);
int dv_infomax_sense_step(dv_ctx *ctx, double x, double y, const double *angles, int n_headings, double *angle_fam,
                          int32_t *best_heading);
int dv_batch_infomax_step_u8(dv_ctx *ctx, const uint8_t *planes, int n_agents, int n_headings, double *angle_fam, int32_t *best_heading);
int dv_batch_infomax_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                                double *angle_fam, int32_t *best_heading, uint32_t *flags);
int dv_infomax_read_weights(dv_ctx *ctx, double *out);
int dv_infomax_set_weights(dv_ctx *ctx, const double *weights);
int dv_infomax_info(dv_ctx *ctx, int *n_hidden, int *n_pixels, int64_t *views_trained, int *finite, int64_t *bytes);
int dv_infomax_end(dv_ctx *ctx);

/* ---- mushroom-body familiarity model --------------------------------------- */
/*
 * A third familiarity model behind the same plug-in seam: the mushroom-body circuit of Ardin, Peng, Mangan, Lagogiannis & Webb
 * (2016).  The view's compared plane p (uint8[h, w] flattened in C order, N = h * w pixels) excites n_kc Kenyon cells through a fixed
 * sparse fan-in, conn int32[n_kc, fan_in] (drawn by the caller; a repeated pixel in a row counts twice):
 *     a_k = sum_j p[conn[k, j]]                                   an integer, at most 255 * fan_in
 *     fired = the n_active cells that come first in the order (larger a first, then lower k): np.argsort(-a, kind="stable")[:n_active]
 *     training on a view: wt[fired] = 0 (wt uint8[n_kc], all 1 after begin);   a scored view: d = sum of wt over its fired cells
 * and the calls report familiarity = (double)(-d): 0.0 for a trained view (the largest possible value), -n_active at most novel.
 * Integers from pixel to score: every figure is exact, whatever the order of the work.  Training ORs the fired sets, so it has no
 * order and is idempotent: train(a) then train(b) is train(a + b) is train(b + a).  The memory is n_kc bytes however long the route.
 * The model lives beside, and independent of, a resident library, landscape, patches, diffuse field and Infomax model.
 *   begin            allocates the model and copies conn.  A model already there is replaced.  DV_ERR_INVALID: NULL conn, a conn entry
 *                    outside [0, h * w), channel outside {0, 1, 2}, h or w < 1, h * w > 65536, n_kc < 1, fan_in outside [1, 16],
 *                    n_active outside [1, n_kc].
 *   train_u8         trains on uint8[n, h, w] planes: every view of a call in one launch (8192 views, or 64 MiB of planes, at a time).
 *   train_from_poses senses the n poses as dv_set_library_from_poses does and trains on their `channel` plane with no host round
 *                    trip; out_views (may be NULL) receives uint8[n, h, w, 3].  DV_ERR_INDEX as dv_sense, and then nothing was
 *                    trained; DV_ERR_INVALID when the sensor's shape is not the model's.
 *   score_u8         familiarity[a] = -d of each of uint8[n, h, w] planes, any n >= 1, one launch.
 *   activity_u8      which cells each of uint8[n, h, w] planes excites: fired uint8[n][n_kc] (1 where the cell fires) and threshold
 *                    int32[n], the least a of a firing cell; either may be NULL.
 *   sense_step       one agent step: senses the n_headings patches at (x, y), scores their `channel` plane in one launch and takes
 *                    the first maximum of angle_fam (np.argmax: integer scores tie).  Any n_headings >= 1.  DV_ERR_INDEX like
 *                    dv_sense_step.
 *   dv_batch_mb_step_u8 / dv_batch_mb_sense_step   an ensemble's step.  (The dv_mb_ prefix is kept to the single model's ten calls; the
 *                    ensemble's two are named apart from it, as the Infomax model's are.)  n_agents members of n_headings headings
 *                    each share the one model (conn, wt); member i owns columns [i * n_headings, (i + 1) * n_headings).
 *                    batch_mb_step_u8 scores uploaded planes uint8[n_agents][n_headings][h][w]; batch_mb_sense_step senses member i
 *                    at (x[i], y[i]) along angles[i][0 .. n_headings): every column's workgroup fills its plane from the landscape
 *                    itself, so no view is written to device memory.  angle_fam[n_agents][n_headings] ((double)(-d), +0.0 for a
 *                    trained view) and best_heading[n_agents] (each member's first maximum, np.argmax: integer scores tie) come
 *                    back from ONE enqueue and ONE wait, whatever n_agents is.  Any n_agents >= 1 and n_headings >= 1 (also > 64
 *                    and > 256); more than 8192 columns (or 64 MiB of uploaded planes) run as launches back to back on the stream.
 *                    A column's value has the bits score_u8 / sense_step give the same patch.  batch_mb_sense_step does not fail
 *                    for a footprint that leaves the landscape: flags[i] (uint32[n_agents]) carries DV_RES_SENSE_ERROR for such a
 *                    member, its best_heading is -1 and its row of angle_fam unspecified; the other members' results are
 *                    untouched.  DV_ERR_STATE without a model or (batch_mb_sense_step) without a sensor; DV_ERR_INVALID for a NULL
 *                    pointer, n_agents < 1, n_headings < 1, a sensor whose shape is not the model's, or n_agents * n_headings
 *                    that does not fit an int.
 *   read_weights / set_weights   copy uint8[n_kc] out and in: what a user saves and restores.  DV_ERR_INVALID for a value other
 *                    than 0 or 1.
 *   info             n_kc, n_pixels, fan_in, n_active, views trained since begin, n_depressed (the number of zero weights: how full
 *                    the memory is), bytes of the weights; zeros without a model; any pointer may be NULL.
 *   end              frees the model; dv_destroy frees it too.
 * Every call but begin, info and end returns DV_ERR_STATE without a model.
 */
int dv_mb_begin(dv_ctx *ctx, int h, int w, int channel, int n_kc, int fan_in, int n_active, const int32_t *conn);
int dv_mb_train_u8(dv_ctx *ctx, const uint8_t *planes, int64_t n);
int dv_mb_train_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n, uint8_t *out_views);
int dv_mb_score_u8(dv_ctx *ctx, const uint8_t *planes, int n, double *familiarity);
int dv_mb_activity_u8(dv_ctx *ctx, const uint8_t *planes, int n, uint8_t *fired, int32_t *threshold);
int dv_mb_sense_step(dv_ctx *ctx, double x, double y, const double *angles, int n_headings, double *angle_fam, int32_t *best_heading);
int dv_batch_mb_step_u8(dv_ctx *ctx, const uint8_t *planes, int n_agents, int n_headings, double *angle_fam, int32_t *best_heading);
int dv_batch_mb_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                           double *angle_fam, int32_t *best_heading, uint32_t *flags);
int dv_mb_read_weights(dv_ctx *ctx, uint8_t *out);
int dv_mb_set_weights(dv_ctx *ctx, const uint8_t *weights);
int dv_mb_info(dv_ctx *ctx, int *n_kc, int *n_pixels, int *fan_in, int *n_active, int64_t *views_trained, int64_t *n_depressed,
               int64_t *bytes);
int dv_mb_end(dv_ctx *ctx);

/* ---- mushroom-body memory banks ---------------------------------------------- */
/*
 * Several memories behind ONE connectivity: the weights are uint8[n_banks][n_kc], bank b at offset b * n_kc.  A bank is a route's
 * memory: the trials of a grid that differ in their training route share the model's connectivity, selection and launches, and each
 * trains and scores through the n_kc bytes of its own bank.  n_banks is 1 after dv_mb_begin; the dv_mb_ and dv_batch_mb_ calls act on
 * bank 0 and touch no other.  A bank table is int32, one entry per view (training) or per member (a step); every entry is checked
 * against [0, n_banks) before anything of the call reaches the device: DV_ERR_INVALID names the first entry out of range, and nothing
 * was trained, scored or uploaded.
 *   set              n_banks >= 1 memories, all weights 1, all view counts 0 (whatever was trained before is dropped).  DV_ERR_OOM
 *                    leaves the model as it was.  dv_mb_begin and dv_mb_end return to one bank.
 *   train_u8 / train_from_poses   as their dv_mb_ twins, with view v depressing bank bank_of_view[v]: the views of all banks share the
 *                    launches (training has no order, and a view writes inside its own bank only).  DV_ERR_INDEX: nothing was trained
 *                    in any bank.
 *   step_u8 / sense_step   as dv_batch_mb_step_u8 / dv_batch_mb_sense_step, with member i scored under bank bank_of_member[i]: one
 *                    enqueue and one wait.
 *   read_weights / set_weights   copy uint8[n_kc] of one bank out and in; DV_ERR_INVALID for a bank outside [0, n_banks) or a value
 *                    other than 0 or 1.
 *   info             n_banks, and per bank the views trained and the zero weights: views_trained and n_depressed are the caller's
 *                    arrays of n_banks entries (ask for n_banks first); any pointer may be NULL.  One bank without a model.
 * Every call but info returns DV_ERR_STATE without a model.
 */
int dv_mbank_set(dv_ctx *ctx, int n_banks);
int dv_mbank_train_u8(dv_ctx *ctx, const uint8_t *planes, int64_t n, const int32_t *bank_of_view);
int dv_mbank_train_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n, const int32_t *bank_of_view,
                              uint8_t *out_views);
int dv_mbank_step_u8(dv_ctx *ctx, const uint8_t *planes, int n_agents, int n_headings, const int32_t *bank_of_member, double *angle_fam,
                     int32_t *best_heading);
int dv_mbank_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                        const int32_t *bank_of_member, double *angle_fam, int32_t *best_heading, uint32_t *flags);
int dv_mbank_read_weights(dv_ctx *ctx, int bank, uint8_t *out);
int dv_mbank_set_weights(dv_ctx *ctx, int bank, const uint8_t *weights);
int dv_mbank_info(dv_ctx *ctx, int *n_banks, int64_t *views_trained, int64_t *n_depressed);

/* ---- mushroom-body population tables ---------------------------------------- */
/*
 * Banks with cells, wiring, quota and compared channel of their own.  A population is (channel, n_kc, fan_in, n_active,
 * conn int32[n_kc][fan_in]); the views' h x w, so n_pixels, stay the ones dv_mb_begin fixed.  A table gives the context n_pops
 * populations and n_banks banks; population_of_bank[b] names bank b's, and several banks may share one (routes x one wiring).  The
 * weights are ragged: bank b holds uint8[n_kc of its population].  While a table is live
 *   - the banked calls (dv_mbank_train_u8, dv_mbank_train_from_poses, dv_lands_mbank_train_from_poses, dv_mbank_step_u8,
 *     dv_mbank_sense_step, dv_lands_mbank_sense_step; with or without a sensor table) take no new argument: view v is trained, or member i
 *     scored, through its bank's own cells, wiring, quota and channel, in the same launches as the views and members of every other bank;
 *   - dv_mbank_read_weights / dv_mbank_set_weights move n_kc bytes of the bank's own population (the 0/1 check runs on that length), and
 *     dv_mbank_info counts each bank's zero weights over its own length;
 *   - the calls that assume the begin's wiring behind bank 0 (dv_mb_train_u8, dv_mb_train_from_poses, dv_mb_score_u8, dv_mb_activity_u8,
 *     dv_mb_sense_step, dv_batch_mb_step_u8, dv_batch_mb_sense_step, dv_mb_read_weights, dv_mb_set_weights) return DV_ERR_STATE, naming
 *     dv_mbpop_clear;
 *   - dv_mb_info keeps describing the model dv_mb_begin made (n_kc, n_pixels, fan_in, n_active, bytes); its two counts, views_trained
 *     and n_depressed, are bank 0's, n_depressed over the cells of bank 0's own population.
 * Without a table every call launches what it launched before there were tables.
 *   set     conn_concat holds population p's int32[n_kc[p]][fan_in[p]], one after another.  DV_ERR_STATE without a model.  Every entry is
 *           checked as dv_mb_begin checks its own -- n_kc in [1, 2^24], fan_in in [1, 16], n_active in [1, n_kc], channel in [0, 2], every
 *           conn value in [0, n_pixels), population_of_bank in [0, n_pops) -- before anything reaches the device: DV_ERR_INVALID names the
 *           population and the entry.  All weights start at 1 and all view counts at 0 (whatever was trained before is dropped).  On an
 *           allocation failure the model, its banks and an earlier table stay as they were.
 *   clear   back to one bank of the begin's population, weights 1.  dv_mbank_set, dv_mb_begin and dv_mb_end drop the table too.
 *   info    n_pops and n_banks (both 0 without a table); per population n_kc, fan_in, n_active, channel (the caller's arrays of n_pops
 *           entries); per bank population_of_bank, views_trained, n_depressed (arrays of n_banks entries); bytes: the table's device
 *           bytes (weights, wirings, descriptors).  Ask for the counts first; any pointer may be NULL.
 */
int dv_mbpop_set(dv_ctx *ctx, int n_pops, const int32_t *n_kc, const int32_t *fan_in, const int32_t *n_active, const int32_t *channel,
                 const int32_t *conn_concat, int n_banks, const int32_t *population_of_bank);
int dv_mbpop_clear(dv_ctx *ctx);
int dv_mbpop_info(dv_ctx *ctx, int *n_pops, int *n_banks, int32_t *n_kc, int32_t *fan_in, int32_t *n_active, int32_t *channel,
                  int32_t *population_of_bank, int64_t *views_trained, int64_t *n_depressed, int64_t *bytes);

/* ---- mushroom-body bank sets ------------------------------------------------ */
/*
 * One selection of firing cells read out through several banks.  A member i of a step carries a set of set_size entries,
 * 1 <= set_size <= DV_MBSET_MAX_BANKS: banks[i][j] in [0, n_banks) (a bank may occur twice) and an int32 coefs[i][j].  For a column
 * (i, a) with fired set F (the model's own selection, unchanged)
 *     d_j = #{k in F : weight of bank banks[i][j] at k is 1},   v = sum_j coefs[i][j] * d_j,   angle_fam[i][a] = (double)(-v)
 * best_heading[i] is the first maximum of angle_fam[i] (the larger value, then the lower heading); a member with a footprint off its
 * landscape gets best_heading -1 and DV_RES_SENSE_ERROR, as in the banked step.  bank_novelty (may be NULL) receives
 * int32[n_agents][n_headings][set_size], the d_j.  Opponent memories are banks {attractive, repulsive} with coefs {1, -gain}; a
 * capacity read-out is one member with eight prefix banks and bank_novelty.
 * Checks, all before anything reaches the device: set_size; every banks entry (DV_ERR_INVALID names it); and a member with
 * sum_j |coefs[i][j]| * n_active > 2^31 - 1 (DV_ERR_INVALID names the member: v could wrap).  One enqueue and one wait, launches as the
 * banked step's; tables are uploaded only when the device does not hold them already.
 *   dv_mbset_step_u8            uploaded planes uint8[n_agents][n_headings][h][w]
 *   dv_mbset_sense_step         sensed on the context's one landscape (refused under live noise rows, as dv_mbank_sense_step)
 *   dv_mbset_lands_sense_step   member i sensed on landscape land_of_member[i] of the set, under the set's sensor table and live noise
 *                               rows where there are any
 * DV_ERR_STATE without a model, and while a population table is live: banks of different populations share no selection (not built).
 */
#define DV_MBSET_MAX_BANKS 8
int dv_mbset_step_u8(dv_ctx *ctx, const uint8_t *planes, int n_agents, int n_headings, int set_size, const int32_t *banks,
                     const int32_t *coefs, double *angle_fam, int32_t *best_heading, int32_t *bank_novelty);
int dv_mbset_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings, int set_size,
                        const int32_t *banks, const int32_t *coefs, double *angle_fam, int32_t *best_heading, uint32_t *flags,
                        int32_t *bank_novelty);
int dv_mbset_lands_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                              int set_size, const int32_t *banks, const int32_t *coefs, const int32_t *land_of_member, double *angle_fam,
                              int32_t *best_heading, uint32_t *flags, int32_t *bank_novelty);

/* ---- Infomax weight banks --------------------------------------------------- */
/*
 * Several Infomax models of one shape and one learning rate in ONE context: the weights are float64[n_banks][n_hidden][h * w], bank b
 * at offset b * n_hidden * h * w.  A bank is a route's model: the trials of a grid that differ in their training route train in one
 * call and step in one call, each through its own bank.  n_banks is 1 after dv_infomax_begin; the dv_infomax_ and dv_batch_infomax_
 * calls act on bank 0 and touch no other.  A bank table is int32, one entry per view (training) or per member (a step); every entry is
 * checked against [0, n_banks) before anything of the call reaches the device: DV_ERR_INVALID names the first entry out of range, and
 * nothing was trained, scored or uploaded.  A table that names a bank whose weights are not finite: DV_ERR_STATE, likewise.
 *   set              n_banks >= 1 banks (at most 65535), every one a copy of w0 (float64[n_hidden * h * w], required), all view counts
 *                    0 (whatever was trained before is dropped).  DV_ERR_OOM leaves the model as it was.  dv_infomax_begin and
 *                    dv_infomax_end return to one bank.
 *   train_u8 / train_from_poses   as their dv_infomax_ twins, with view v trained into bank bank_of_view[v].  Every bank's views are
 *                    taken in the order they have in the call, and the R chains advance in lockstep: step s of the call is every
 *                    bank's s-th view, in the three launches one chain's step takes.  A bank's weights after the call have the bits
 *                    dv_infomax_train_u8 gives on that bank's views alone from the same weights; a bank that gets no view keeps its
 *                    bits.  n = 0 is legal for train_u8.  DV_ERR_INDEX (train_from_poses): nothing was trained in any bank.
 *                    DV_ERR_STATE after the call: the message names the first bank of the call whose weights are no longer finite,
 *                    and the learning rate; the other banks hold their own chains' weights and go on working.
 *   step_u8 / sense_step   as dv_batch_infomax_step_u8 / dv_batch_infomax_sense_step, with member i scored under bank
 *                    bank_of_member[i]: the members may come in any bank order, the results come in the caller's order, from one
 *                    enqueue and one wait.  A column's value has the bits dv_infomax_score_u8 gives the same patch on a model that
 *                    holds that bank's weights.  flags, the sensor-shape check and DV_RES_SENSE_ERROR per member as
 *                    dv_batch_infomax_sense_step.
 *   read_weights / set_weights   copy float64[n_hidden][h * w] of one bank out and in; DV_ERR_INVALID for a bank outside
 *                    [0, n_banks).  set_weights with finite weights makes a bank that diverged usable again.
 *   info             n_banks, and per bank the views trained and whether the weights are finite: views_trained and finite are the
 *                    caller's arrays of n_banks entries (ask for n_banks first); any pointer may be NULL.  One bank without a model.
 * Every call but info returns DV_ERR_STATE without a model.
 */
int dv_ibank_set(dv_ctx *ctx, int n_banks, const double *w0);
int dv_ibank_train_u8(dv_ctx *ctx, const uint8_t *planes, int64_t n, const int32_t *bank_of_view);
int dv_ibank_train_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n, const int32_t *bank_of_view,
                              uint8_t *out_views);
int dv_ibank_step_u8(dv_ctx *ctx, const uint8_t *planes, int n_agents, int n_headings, const int32_t *bank_of_member, double *angle_fam,
                     int32_t *best_heading);
int dv_ibank_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                        const int32_t *bank_of_member, double *angle_fam, int32_t *best_heading, uint32_t *flags);
int dv_ibank_read_weights(dv_ctx *ctx, int bank, double *out);
int dv_ibank_set_weights(dv_ctx *ctx, int bank, const double *weights);
int dv_ibank_info(dv_ctx *ctx, int *n_banks, int64_t *views_trained, int32_t *finite);

/* ---- Infomax network tables -------------------------------------------------- */
/*
 * Banks with hidden units, learning rate, initial weights and compared channel of their own.  A network is (channel, n_hidden,
 * learning_rate, W0 float64[n_hidden][h * w]); the views' h x w, so n_pixels, stay the ones dv_infomax_begin fixed.  A table gives the
 * context n_nets networks and n_banks banks; network_of_bank[b] names bank b's, and several banks may share one (routes x one network).
 * Bank b starts as a copy of its network's W0.  The weights are ragged: bank b holds float64[n_hidden of its network][h * w].  While a
 * table is live
 *   - the banked calls (dv_ibank_train_u8, dv_ibank_train_from_poses, dv_lands_ibank_train_from_poses, dv_ibank_step_u8,
 *     dv_ibank_sense_step, dv_lands_ibank_sense_step; with or without a sensor table) take no new argument: view v is trained into bank
 *     bank_of_view[v] through that bank's n_hidden and channel at rate = learning_rate / n_pixels, in the same three launches per
 *     lockstep step as every other bank's chain, and member i is scored in the same launches as the members of every other bank;
 *   - a bank's weights after training have the bits of a context begun with its network (dv_infomax_begin(h, w, channel, n_hidden,
 *     learning_rate, W0)) and trained on that bank's views alone, in their order; a bank that gets no view keeps its bits; a column of a
 *     step has the bits dv_infomax_score_u8 gives the same patch on that context;
 *   - dv_ibank_read_weights / dv_ibank_set_weights move n_hidden x n_pixels doubles of the bank's own network; dv_ibank_info is unchanged;
 *   - divergence is per bank: DV_ERR_STATE names the bank and ITS OWN learning rate, the other banks hold their chains' weights and go on
 *     working, and dv_ibank_set_weights with finite weights heals the bank;
 *   - the calls that assume the begin's shape behind bank 0 (dv_infomax_train_u8, dv_infomax_train_from_poses, dv_infomax_score_u8,
 *     dv_infomax_sense_step, dv_infomax_read_weights, dv_infomax_set_weights, dv_batch_infomax_step_u8, dv_batch_infomax_sense_step)
 *     return DV_ERR_STATE, naming dv_inet_clear;
 *   - dv_infomax_info keeps describing the model dv_infomax_begin made (n_hidden, n_pixels, bytes); its two counts, views_trained and
 *     finite, are bank 0's.
 * Without a table every call launches what it launched before there were tables.
 *   set     w0_concat holds network p's float64[n_hidden[p]][h * w], one after another.  DV_ERR_STATE without a model.  Every entry is
 *           checked as dv_infomax_begin checks its own -- n_hidden in [1, 2^20], learning_rate finite and > 0, channel in [0, 2],
 *           network_of_bank in [0, n_nets), n_banks in [1, 65535] -- before anything reaches the device: DV_ERR_INVALID names the network
 *           and the entry.  All view counts start at 0 (whatever was trained before is dropped).  Everything is allocated and every copy
 *           waited for before the table is installed: on a failure the model, its banks and an earlier table stay as they were.
 *   clear   back to one bank of the begin's network at the W0 dv_infomax_begin was given.  dv_ibank_set, dv_infomax_begin and
 *           dv_infomax_end drop the table too.
 *   info    n_nets and n_banks (both 0 without a table); per network n_hidden, learning_rate, channel (the caller's arrays of n_nets
 *           entries); per bank network_of_bank, views_trained, finite (arrays of n_banks entries); bytes: the table's device bytes
 *           (weights, h, u, partial sums, flags, descriptors).  Ask for the counts first; any pointer may be NULL.
 */
int dv_inet_set(dv_ctx *ctx, int n_nets, const int32_t *n_hidden, const double *learning_rate, const int32_t *channel,
                const double *w0_concat, int n_banks, const int32_t *network_of_bank);
int dv_inet_clear(dv_ctx *ctx);
int dv_inet_info(dv_ctx *ctx, int *n_nets, int *n_banks, int32_t *n_hidden, double *learning_rate, int32_t *channel,
                 int32_t *network_of_bank, int64_t *views_trained, int32_t *finite, int64_t *bytes);

/* ---- landscape sets ---------------------------------------------------------- */
/*
 * Several HSV landscapes of any shapes resident together in ONE context, and a landscape index per pose in the sensed calls of the
 * banked models: the landscape replicates of a grid (and, with a bank per route, their routes) train in one call and step in one call.
 * The set is one allocation with the landscapes back to back, no padding.  The sensor geometry, the level table and the mask stay the
 * context's one configuration (dv_configure_sensor), shared by all landscapes of the set unless a sensor table gives every landscape
 * its own (dv_sensors_set, below).  dv_set_landscape's landscape and every call
 * that reads it are untouched by a set, and the set by them: dv_set_landscape, dv_mb_end and dv_infomax_end leave the set alone;
 * dv_destroy frees it.  A landscape table is int32, one entry per pose or view (lands_sense, training) or per member (a step); every
 * entry is checked against [0, n_lands) before anything of the call reaches the device: DV_ERR_INVALID names the first entry out of
 * range, and nothing was trained, scored, uploaded or reallocated.  DV_ERR_STATE without a set.
 *   set              lands: uint8, landscape l is [rows[l]][cols[l]][3] and follows landscape l - 1 directly.  n_lands >= 1, channels 3.
 *                    The replacement is built first and put in place when complete: DV_ERR_OOM leaves the old set as it was.
 *   clear            no set; its memory is freed.
 *   info             n_lands (0: no set), the shapes (the caller's arrays of n_lands entries: ask for n_lands first) and the bytes of
 *                    the set; any pointer may be NULL.
 *   sense            dv_sense with pose v on landscape land_of_pose[v].  A negative index wraps by the pose's own rows and cols; a
 *                    footprint past the end of its own landscape: DV_ERR_INDEX, and the message names the first such pose.
 *   dv_lands_mbank_train_from_poses / dv_lands_ibank_train_from_poses   as dv_mbank_ / dv_ibank_train_from_poses, view v sensed on landscape
 *                    land_of_view[v]: the same slabs, the same chains, and DV_ERR_INDEX trains nothing in any bank.
 *   dv_lands_mbank_sense_step / dv_lands_ibank_sense_step   as dv_mbank_ / dv_ibank_sense_step, member i sensed on landscape land_of_member[i]: one enqueue,
 *                    one wait, results in the caller's order, DV_RES_SENSE_ERROR for a member whose footprint leaves its own landscape.
 */
int dv_lands_set(dv_ctx *ctx, const uint8_t *lands, const int32_t *rows, const int32_t *cols, int n_lands, int channels);
int dv_lands_clear(dv_ctx *ctx);
int dv_lands_info(dv_ctx *ctx, int *n_lands, int32_t *rows, int32_t *cols, int64_t *bytes);
int dv_lands_sense(dv_ctx *ctx, const double *x, const double *y, const double *angle, const int32_t *land_of_pose, int n, uint8_t *out);
int dv_lands_mbank_train_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n,
                                    const int32_t *bank_of_view, const int32_t *land_of_view, uint8_t *out_views);
int dv_lands_ibank_train_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n,
                                    const int32_t *bank_of_view, const int32_t *land_of_view, uint8_t *out_views);
int dv_lands_mbank_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                              const int32_t *bank_of_member, const int32_t *land_of_member, double *angle_fam, int32_t *best_heading,
                              uint32_t *flags);
int dv_lands_ibank_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                              const int32_t *bank_of_member, const int32_t *land_of_member, double *angle_fam, int32_t *best_heading,
                              uint32_t *flags);

/* ---- sensor tables: a sensor configuration per landscape of the set ----------- */
/*
 * Entry l of a sensor table is the sensor that landscape l of the live landscape set is sensed with: sensor_pixel_dimensions (pw[l],
 * ph[l]), mask_middle_n mask_n[l] and a level table uint8[3][256] of its own (luts: the entries' tables back to back).  The sensor's
 * w x h stays the context's one for all entries (dv_configure_sensor): the one-value models and the route view store are built on it.
 * A trial that uses two sensors on one landscape enters that landscape into the set twice.
 * With a table, every call that takes a landscape table senses a pose under its landscape's entry, with no new argument:
 * dv_lands_sense, dv_lands_mbank_ / dv_lands_ibank_train_from_poses, dv_lands_mbank_ / dv_lands_ibank_sense_step, and
 * dv_rviews_set_from_poses / dv_rviews_sense_step / dv_rviews_scene with a land_of_* table.  The footprint that must stay on a pose's
 * landscape is its entry's own, (w pw) x (h ph).  A call with land_of_* == NULL, and every call that takes no landscape table, senses
 * the context's landscape under the context's sensor, table or not; with no table every call does what it did before.
 *   set              n == n_lands of the live set (DV_ERR_STATE without a set or a configured sensor, DV_ERR_INVALID otherwise).  Every
 *                    entry is checked as dv_configure_sensor checks its own -- pw, ph >= 1, pw * ph <= 4096, 0 <= mask_n <= w / 2 -- and
 *                    DV_ERR_INVALID names the entry.  The replacement is built first: an error leaves the old table as it was.
 *   clear            no table: the context's one sensor for every landscape again.
 *   info             n (0: no table) and the entries (the caller's arrays of n, luts of n * 768: ask for n first); any pointer may be NULL.
 * dv_lands_set and dv_lands_clear drop a live table (the entries it belonged to are gone), as does a dv_configure_sensor that changes
 * w x h; dv_destroy frees it.
 */
int dv_sensors_set(dv_ctx *ctx, const int32_t *pw, const int32_t *ph, const int32_t *mask_n, const uint8_t *luts, int n);
int dv_sensors_clear(dv_ctx *ctx);
int dv_sensors_info(dv_ctx *ctx, int *n, int32_t *pw, int32_t *ph, int32_t *mask_n, uint8_t *luts);

/* ---- noise rows: sensor noise on landscape sets, a reproducible draw per sensing */
/*
 * The sensed views are a deterministic function of the pose.  With noise rows live, every sensed call that takes a landscape table
 * adds an integer draw to the S and V of every sensor pixel, with no new argument: dv_lands_sense, dv_lands_mbank_ /
 * dv_lands_ibank_train_from_poses, dv_lands_mbank_ / dv_lands_ibank_sense_step, and dv_rviews_set_from_poses and the dv_rviews_ /
 * dv_rvwin_ / dv_rvssd_ / dv_rvssdw_ sensed steps and scenes with a land_of_* table.  Row i = (keys[i], amp_s[i], amp_v[i]) belongs to
 * member i of a step or scene call, or to view / pose i of a training, store or dv_lands_sense call.  For sensor pixel j = bi w + bj
 * (row-major) of the row's heading a (a = 0 where the call has one pose per row), with P = w h and uint64 arithmetic that wraps:
 *     base = splitmix64(key + seed * 0x9E3779B97F4A7C15)       word = splitmix64(base + (a * P + j))
 *     d_S  = word & 0xFFFFFFFF, d_V = word >> 32               n_c = ((d_c * (2 * amp_c + 1)) >> 32) - amp_c, in [-amp_c, +amp_c]
 *     S'   = clamp(S + n_S, 0, 255), V' = clamp(V + n_V, 0, 255)
 * S and V are the sensor pixel's values after the pixel block's rule and before the level tables; the hue is the noiseless model's
 * (a zero-saturation pixel has hue 0, decided on the noiseless S); the level tables (the pose's own entry's under a sensor table) and
 * the mask follow, so masked pixels stay 0.  A row of zero amplitudes gives the noiseless bytes.  The draw depends on the key and the
 * pixel's place within the row, not on the row's index or on who else is in the call.  A footprint off its landscape is the error it is
 * without rows.
 *   rows             n >= 1 rows replace the live ones; built first, in place only when complete.  An unchanged table is not uploaded
 *                    again.  DV_ERR_STATE without a configured sensor.
 *   clear            no rows: every call launches exactly what it launched before.
 *   info             n (0: none), the seed and the rows (the caller's arrays of n: ask for n first); any pointer may be NULL.
 * While rows are live, a sensed call whose landscape table has not n entries is refused before anything reaches the device
 * (DV_ERR_INVALID names both counts); a sensed call of the banked models or the route view store WITHOUT a landscape table is refused
 * with DV_ERR_STATE (it would sense without noise), as is dv_lands_mbank_sense_step under a population table; the uploaded-patch calls
 * (*_u8), the library path (dv_step*, dv_sense_step*), dv_sense and the single-agent calls are untouched and noiseless.  dv_lands_set,
 * dv_lands_clear and dv_sensors_clear leave the rows alone; a dv_configure_sensor that changes w x h drops them (P enters the
 * counter); dv_destroy frees them.
 */
int dv_noise_rows(dv_ctx *ctx, uint64_t seed, const uint64_t *keys, const uint8_t *amp_s, const uint8_t *amp_v, int64_t n);
int dv_noise_clear(dv_ctx *ctx);
int dv_noise_info(dv_ctx *ctx, int64_t *n, uint64_t *seed, uint64_t *keys, uint8_t *amp_s, uint8_t *amp_v);

/* ---- route view store: perfect-memory members on their own routes ------------ */
/*
 * The sensed views of R training routes side by side as raw HSV bytes, and a step that scores every member's headings against the
 * views of ITS OWN route only: the sads_hsv model (navsim/util.pyx:31-73) for ensembles of trials that differ in their training route
 * and their landscape.  Route r is views [first[r], first[r + 1]) (first: int64[n_routes + 1], first[0] = 0, at least 2 views a
 * route).  The store stands beside the library (dv_set_library and every dv_step* / dv_sense_step* call work unchanged beside it and
 * after it is cleared); its layout depends on neither the data nor a weight.  Views of h x w with h * w <= 4096.
 * A step's tables are route_of_member (int32[n_agents], in [0, n_routes)), chem_weights (double[n_agents], in [0, 1]) and, for
 * sensed calls on a live landscape set, land_of_member (int32[n_agents]; NULL: the context's one landscape).  Every entry, and first,
 * is checked before anything of the call reaches the device: DV_ERR_INVALID names it and nothing changes.  DV_ERR_STATE without a store.
 *   set_u8           views: uint8[first[n_routes]][h][w][3].  The replacement is built first: an error leaves the old store as it was.
 *   set_from_poses   senses the n = first[n_routes] views in one call, on the context's landscape or view v on landscape land_of_view[v]
 *                    of the live set; out_views (may be NULL) receives them.  DV_ERR_INDEX names the first view whose footprint leaves
 *                    its own landscape, and the store stays as it was.
 *   step_u8          patches: uint8[n_agents][n_headings][h][w][3].  angle_fam[i * n_headings + a]: the reference's value (bit for
 *                    bit) of the most familiar view of member i's route for heading a, angle_view (may be NULL) the first view that
 *                    attains it (an index within the route), best_heading[i] the first maximum of member i's row (np.argmax).  Any
 *                    n_headings >= 1, any n_agents (scored in slabs of what a 64 MiB score buffer holds; DEJAVU_RVIEWS_SLAB = columns,
 *                    read at dv_create, sets another slab size for tests).  flags: DV_RVIEWS_EXACT scores every view as the reference's
 *                    sequential sum (as dv_set_exact does); the default finds the candidates with exact integer sums and scores
 *                    those again, with the same results.
 *   sense_step       step_u8 with the patches sensed at (x[i], y[i]) along angles[i * n_headings + a]: one enqueue, one wait.
 *                    member_flags[i] carries DV_RES_SENSE_ERROR for a member whose footprint leaves its own landscape (its row is
 *                    unspecified, its best_heading -1); the others are scored.
 *   scene_u8 / scene scene_familiarity of the members: per view of member i's route the least value over its headings, the members'
 *                    rows back to back in scene_fam (n_out doubles: the sum of the members' route lengths).  A member with
 *                    DV_RES_SENSE_ERROR gets a row of +inf.  member_flags may be NULL.
 *   info             n_routes (0: no store), first (the caller's n_routes + 1 entries: ask for n_routes first), the views' shape and
 *                    the bytes of the store; any pointer may be NULL.
 *   clear            no store; its memory is freed.
 */
#define DV_RVIEWS_EXACT 1u
int dv_rviews_set_u8(dv_ctx *ctx, const uint8_t *views, const int64_t *first, int n_routes, int h, int w);
int dv_rviews_set_from_poses(dv_ctx *ctx, const double *x, const double *y, const double *angle, int64_t n, const int64_t *first,
                             int n_routes, const int32_t *land_of_view, uint8_t *out_views);
int dv_rviews_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member,
                      const double *chem_weights, uint32_t flags, double *angle_fam, int64_t *angle_view, int32_t *best_heading);
int dv_rviews_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                         const int32_t *route_of_member, const double *chem_weights, const int32_t *land_of_member, uint32_t flags,
                         double *angle_fam, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);
int dv_rviews_scene_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member,
                       const double *chem_weights, int64_t n_out, double *scene_fam);
int dv_rviews_scene(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                    const int32_t *route_of_member, const double *chem_weights, const int32_t *land_of_member, int64_t n_out,
                    double *scene_fam, uint32_t *member_flags);
int dv_rviews_info(dv_ctx *ctx, int *n_routes, int64_t *first, int *h, int *w, int64_t *bytes);
int dv_rviews_clear(dv_ctx *ctx);

/* ---- windowed steps on the route view store: perfect memory with a temporal window ---- */
/*
 * dv_rviews_step_u8 / dv_rviews_sense_step with member i scored against views [win_lo[i], win_hi[i]) of its own route only (sequence-
 * aware matching: the views a few places behind and ahead of the one the member matched last).  angle_fam is the reference's value bit
 * for bit of the most familiar view INSIDE the window, angle_view (may be NULL) the least route-relative index that attains it (so
 * win_lo[i] <= angle_view < win_hi[i]), best_heading and member_flags as in the unwindowed calls: what the unwindowed step gives on
 * the slice of the route alone, with win_lo[i] added to its view indices.  flags: DV_RVIEWS_EXACT as in dv_rviews_step_u8.
 * Beside the unwindowed calls' checks, for every member 0 <= win_lo[i] < win_hi[i] <= the views of its route and
 * win_hi[i] - win_lo[i] <= DV_RVWIN_MAX_VIEWS, else DV_ERR_INVALID names member i and its values; DV_ERR_STATE without a store.  A
 * refused call changes nothing: the store, the tables the unwindowed calls keep on the device and their results stay as they were.
 * A call is the sensing launch, one launch for the patches' byte planes, ONE scoring launch (no score buffer) and the deciding launch.
 */
#define DV_RVWIN_MAX_VIEWS 512
int dv_rvwin_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member,
                     const double *chem_weights, const int32_t *win_lo, const int32_t *win_hi, uint32_t flags,
                     double *angle_fam, int64_t *angle_view, int32_t *best_heading);
int dv_rvwin_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                        const int32_t *route_of_member, const double *chem_weights, const int32_t *land_of_member,
                        const int32_t *win_lo, const int32_t *win_hi, uint32_t flags,
                        double *angle_fam, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);

/*
 * Re-localisation inside the windowed step.  dv_rvreloc_step_u8 / dv_rvreloc_sense_step are dv_rvwin_step_u8 / dv_rvwin_sense_step
 * with a threshold per member, reloc_below (double[n_agents], in the unit of angle_fam, so at most h * w), behind win_hi; member_flags
 * (uint32[n_agents], not NULL) is an output of both.  THE RULE: once the windowed scores of the step exist, a member that is not
 * flagged DV_RES_SENSE_ERROR is LOST iff max_a angle_fam_window[a] < reloc_below[i] -- a strict < on the doubles as they are, so -inf
 * never triggers and +inf always does.  A lost member's row (angle_fam, angle_view, its part in best_heading) is the whole-route step's
 * bit for bit, what dv_rviews_step_u8 gives at the same patches (more than 256 candidates included); nothing of the windowed attempt
 * remains in it, and its flag word carries DV_RES_RELOCALISED.  Every other member's row is dv_rvwin_*'s bit for bit.
 * Checks: the windowed calls', and DV_ERR_INVALID naming the member for a NaN in reloc_below (and for n_headings above 32768); all
 * of them run before anything reaches the device, and a refused call changes nothing (see dv_rvwin_*).
 * A call is ONE enqueue and ONE wait, and the host reads nothing in between: the sensing launch, the byte planes, the windowed scoring
 * launch, then per group of consecutive members whose columns fit the score buffer of the unwindowed calls (64 MiB, or
 * DEJAVU_RVIEWS_SLAB columns) a launch that applies the rule and writes the lost columns' plan on the device and the unwindowed
 * calls' scoring launches on that plan (grids sized for "every member lost"; a workgroup past the device's counts returns at once),
 * the deciding launch and one copy out.  DV_RVIEWS_EXACT: the rule reads the exact windowed values and the lost columns take the
 * exact pass.
 */
int dv_rvreloc_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member,
                       const double *chem_weights, const int32_t *win_lo, const int32_t *win_hi, const double *reloc_below,
                       uint32_t flags, double *angle_fam, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);
int dv_rvreloc_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                          const int32_t *route_of_member, const double *chem_weights, const int32_t *land_of_member,
                          const int32_t *win_lo, const int32_t *win_hi, const double *reloc_below, uint32_t flags,
                          double *angle_fam, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);

/* ---- SSD on the route view store: exact sum of squared differences of one channel ---- */
/*
 * The reference's `ssds` (navsim/util.pyx:171-184) of channel `channel` (0, 1 or 2: H, S or V; one value per call) between every
 * member's patches and the views of ITS OWN route of the live store (dv_rviews_set_u8 / dv_rviews_set_from_poses, unchanged), on
 * the int8 matrix cores: sum (a - b)^2 = sum a'^2 + sum b'^2 - 2 sum a' b' with a' = a - 128, b' = b - 128, in integers, so every
 * value is the exact integer the reference's float64 loop gives and ties are decided by index alone.  The store is read as it lies;
 * nothing of it, and nothing dv_rviews_* keeps on the device, is written.
 *   step_u8          patches: uint8[n_agents][n_headings][h][w][3].  angle_ssd[i * n_headings + a]: the least ssds(patch[..., channel],
 *                    view[..., channel]) over the views of member i's route (an integer below 2^31, as a double), angle_view (may be
 *                    NULL) the LEAST route-relative view index that attains it, best_heading[i] the FIRST heading with the least
 *                    angle_ssd (np.argmax(-angle_ssd)).  Any n_headings >= 1, any n_agents.
 *   sense_step       step_u8 with the patches sensed as dv_rviews_sense_step senses them (landscape sets and sensor tables included):
 *                    one enqueue, one wait.  member_flags[i] carries DV_RES_SENSE_ERROR for a member whose footprint leaves its own
 *                    landscape (its row is unspecified, its best_heading -1); the others are scored.
 *   scene_u8 / scene per view of member i's route the LARGEST ssds over its headings (-scene_ssd is the reference's scene_familiarity),
 *                    the members' rows back to back as in dv_rviews_scene (n_out doubles).  A member with DV_RES_SENSE_ERROR gets a
 *                    row of -inf.  member_flags may be NULL.
 * Checks: dv_rviews_*'s and 0 <= channel <= 2, all before anything reaches the device; DV_ERR_INVALID names the entry and a refused
 * call changes nothing; DV_ERR_STATE without a store.  The view norms are worked out at the first call on a (store, channel) and kept
 * until the store is replaced or cleared.
 */
int dv_rvssd_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member, int channel,
                     double *angle_ssd, int64_t *angle_view, int32_t *best_heading);
int dv_rvssd_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                        const int32_t *route_of_member, const int32_t *land_of_member, int channel,
                        double *angle_ssd, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);
int dv_rvssd_scene_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member, int channel,
                      int64_t n_out, double *scene_ssd);
int dv_rvssd_scene(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                   const int32_t *route_of_member, const int32_t *land_of_member, int channel,
                   int64_t n_out, double *scene_ssd, uint32_t *member_flags);

/* ---- NCC on the route view store: the correlation coefficient of one channel ---- */
/*
 * dv_rvssd_*'s calls, argument for argument, with the correlation coefficient (zero-mean normalised cross-correlation) in place of the
 * SSD: invariant to the gain and offset of a view.  For a patch plane a and a stored view b of channel `channel`, P = h w pixels, in
 * exact integers
 *     Sa = sum a   Sb = sum b   Saa = sum a^2   Sbb = sum b^2   Sab = sum a b
 *     num = P Sab - Sa Sb      Va = P Saa - Sa^2      Vb = P Sbb - Sb^2
 *     q = 0.0 if Va == 0 or Vb == 0 (a constant plane correlates with nothing), else
 *     q = clip(double(num) / sqrt(double(Va) * double(Vb)), -1, 1): one IEEE double product, one square root, one quotient, in that order.
 * The cross term is dv_rvssd_*'s int8 GEMM on a - 128 and b - 128 (num, Va and Vb do not change), the epilogue is in 64-bit integers
 * (the three reach 2^38; their conversions to double are exact), and every pair is evaluated: the values are the statement's bits.
 *   step_u8          angle_ncc[i * n_headings + a]: the LARGEST q over the views of member i's route, angle_view (may be NULL) the
 *                    LEAST route-relative view index that attains it, best_heading[i] the FIRST heading with the largest angle_ncc
 *                    (np.argmax(angle_ncc)).  Any n_headings >= 1, any n_agents.
 *   sense_step       step_u8 with the patches sensed as dv_rviews_sense_step senses them (landscape sets, sensor tables and noise rows
 *                    included): one enqueue, one wait.  member_flags[i] carries DV_RES_SENSE_ERROR for a member whose footprint leaves
 *                    its own landscape (its row is unspecified, its best_heading -1); the others are scored.
 *   scene_u8 / scene per view of member i's route the LEAST q over its headings (what the reference's loop leaves in scene_familiarity),
 *                    the members' rows back to back as in dv_rviews_scene (n_out doubles).  A member with DV_RES_SENSE_ERROR gets a
 *                    row of +inf.  member_flags may be NULL.
 * Checks: dv_rvssd_*'s, all before anything reaches the device.  The view statistics (sum and sum of squares per view) are worked out at
 * the first call on a (store, channel) and kept until the store is replaced or cleared, apart from dv_rvssd_*'s norms; nothing that
 * dv_rvssd_* keeps is written.  No floating-point atomics and nothing that depends on the order of the workgroups.
 */
int dv_rvncc_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member, int channel,
                     double *angle_ncc, int64_t *angle_view, int32_t *best_heading);
int dv_rvncc_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                        const int32_t *route_of_member, const int32_t *land_of_member, int channel,
                        double *angle_ncc, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);
int dv_rvncc_scene_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member, int channel,
                      int64_t n_out, double *scene_ncc);
int dv_rvncc_scene(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                   const int32_t *route_of_member, const int32_t *land_of_member, int channel,
                   int64_t n_out, double *scene_ncc, uint32_t *member_flags);

/* ---- SSD on the route view store with a temporal window, and re-localisation inside the step ---- */
/*
 * dv_rvssd_step_u8 / dv_rvssd_sense_step with member i scored against views [win_lo[i], win_hi[i]) of its own route only: what the
 * unwindowed call gives on that slice of the route alone, with win_lo[i] added to its view indices (so win_lo[i] <= angle_view <
 * win_hi[i]); every value an exact integer, ties by index alone.  A call is the sensing launch, the operand rows, ONE scoring launch in
 * the caller's column order (no sort, no atomics, no unsort) and the deciding launch.
 * reloc_below (double[n_agents], or NULL: no loss test), in the unit of the model's familiarity, -SSD, so useful values are <= 0.  THE
 * RULE: a member that is not flagged DV_RES_SENSE_ERROR is LOST iff max_a(-angle_ssd_window[a]) < reloc_below[i] -- a strict < on the
 * doubles as they are, so -inf never triggers and +inf always does.  A lost member's row (angle_ssd, angle_view, its best_heading) is
 * dv_rvssd_step_u8's on its whole route, bit for bit, and its flag word carries DV_RES_RELOCALISED; every other member's row is the
 * windowed one.  The loss test, the plan of the lost columns, their whole-route scoring and the write-back are enqueued between the
 * windowed scoring and the deciding launch: ONE enqueue and ONE wait, and the host reads nothing in between.
 * member_flags (uint32[n_agents]): an output; step_u8 takes NULL when reloc_below is NULL.
 * Checks, all before anything reaches the device (a refused call changes nothing): dv_rvssd_*'s; dv_rvwin_*'s window rule (0 <=
 * win_lo[i] < win_hi[i] <= the views of the route, at most DV_RVWIN_MAX_VIEWS views; DV_ERR_INVALID names member, window and route);
 * with reloc_below, DV_ERR_INVALID naming the member for a NaN, and for n_headings above 32768.  DV_ERR_STATE without a store.
 */
int dv_rvssdw_step_u8(dv_ctx *ctx, const uint8_t *patches, int n_agents, int n_headings, const int32_t *route_of_member,
                      const int32_t *win_lo, const int32_t *win_hi, const double *reloc_below, int channel,
                      double *angle_ssd, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);
int dv_rvssdw_sense_step(dv_ctx *ctx, const double *x, const double *y, const double *angles, int n_agents, int n_headings,
                         const int32_t *route_of_member, const int32_t *land_of_member, const int32_t *win_lo, const int32_t *win_hi,
                         const double *reloc_below, int channel,
                         double *angle_ssd, int64_t *angle_view, int32_t *best_heading, uint32_t *member_flags);

/* ---- measurement ------------------------------------------------------- */
/* hipEvent pair on the context's stream around whatever is enqueued between the two calls. */
int dv_timer_start(dv_ctx *ctx);
int dv_timer_stop(dv_ctx *ctx, float *elapsed_ms);
/* enable = n > 0: bracket every n-th launch of the scoring kernel with hipEvents (1 = every launch; an event pair
 * costs a few microseconds of stream time, so throughput runs sample); 0: off. */
int dv_profile_kernel(dv_ctx *ctx, int enable);
/* Sum and count of the bracketed scoring-kernel launches since the last read; resets. */
int dv_profile_read(dv_ctx *ctx, double *total_ms, int64_t *n_launches);
/* Workgroup shape of the scoring kernel in use for steps of n_headings headings on the resident library (1..5: forms
 * of the byte-plane kernels, csrc/dejavu_hip.hip:launch_tiles_apad; 6: the bit-plane matrix-core kernel k_sad_mfma_dual (mixed layout: + a v_sad_u8 pass over the saturation byte planes);
 * 0 = not timed yet, or not applicable to this library). */
int dv_workgroup_shape(dv_ctx *ctx, int n_headings, int *shape);
/* Streaming-read microbenchmark over n_bytes of device memory (achievable HBM ceiling). */
int dv_stream_read_gbps(dv_ctx *ctx, int64_t n_bytes, int iters, double *gbps);

/*
 * roctx ranges (rocprofv3 --marker-trace): with DEJAVU_ROCTX=1 in the environment the library brackets the phases of a
 * step ("dv:sense", "dv:score", "dv:finish", "dv:wait") and callers can add their own (navsim_amd/sharded.py wraps the
 * per-step exchange in "dv:exchange").  No-ops otherwise; libroctx64.so is looked up at run time.
 */
int dv_range_push(const char *name);
int dv_range_pop(void);

/* 1 when the resident patches have every byte on one of the library's levels (or outside their range), i.e. the last
 * coefficient prep allowed the fp4 form of the matrix-core kernel; 0 when a byte lies strictly inside a gap (the int8
 * form scored or will score them); DV_ERR_STATE when the library has no fp4 form or no patches were prepared for it.
 * Waits for the stream.  Diagnostic: the kernel itself reads the same word on the device, nothing on the host decides.
 * (The reference has no counterpart; its patches come out of the quantiser of NavBySceneFamiliarity.py:176-186.) */
int dv_patches_on_level(dv_ctx *ctx);

/* Form of the last integer scoring pass, as flags: DV_FORM_MATRIX_CORES (bit-plane library on the matrix cores, workgroup
 * shape 6), DV_FORM_FP4 (its fp4 coefficients: the prep's patches were on-level), DV_FORM_FUSED_FINISH (the kernel
 * finished its scores itself; the step ended in k_fold), DV_FORM_CODES (the fp4 form's body read the value rows as 3-bit level
 * codes, the code tiles of dv_lib_info.code_tile_bytes), DV_FORM_CONSUMERS8 (... in the registers of all eight waves of a workgroup,
 * items of 16 view groups: DEJAVU_LREG8).  Bits DV_FORM_BODY_SHIFT .. of a matrix-core pass name the kernel body the host launched,
 * 1 + its index in DV_FORM_BODY_NAMES (0: none); with the fp4 flag clear the launch took that body's int8 form.
 * Waits for the stream when the fp4 word has to be read.
 * Diagnostic for benchmarks and tests; negative on error. */
#define DV_FORM_MATRIX_CORES 1
#define DV_FORM_FP4 2
#define DV_FORM_FUSED_FINISH 4
#define DV_FORM_CODES 8
#define DV_FORM_CONSUMERS8 16
#define DV_FORM_BODY_SHIFT 8
#define DV_FORM_BODY_BITS 5
#define DV_FORM_BODY_NAMES "Ring Ring2 RingA RingB Lc LcShort LcCode LcReg LcRegCode LcRegCode8 Lc2Tiles Lc2TilesCode Lc22"
int dv_scoring_form(dv_ctx *ctx);

const char *dv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DEJAVU_H */

/* parasitoid_hip.h -- C ABI of libparasitoid_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the drift-diffusion forward solver of
 * mountaindust/Parasitoids.  Each entry point names the reference interface it
 * replaces (file:line relative to the reference repository).  Plain pointers and
 * sizes only; all inputs are caller-owned host buffers that are copied before
 * the call returns and never modified; outputs go to caller-allocated buffers
 * sized from a preceding count call (two-phase COO output).
 *
 * Every function returns PS_OK (0) or a negative error class; ps_last_error()
 * gives the message of the last failure on the calling thread.  One handle =
 * one device + one HIP stream; a handle is not thread-safe, different handles
 * are independent.  No HIP call is made at library load (fork-safe: the
 * reference forks a multiprocessing pool before it touches the GPU,
 * Run.py:422-425, Bayes_Run.py:706).
 */
#ifndef PARASITOID_HIP_H
#define PARASITOID_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_OK 0
#define PS_ERR_NO_DEVICE (-1)   /* no gfx950 device / HIP runtime unusable          */
#define PS_ERR_OOM (-2)         /* device allocation failed (cuda_lib.py:31,:72,:108,:159 asserts) */
#define PS_ERR_BAD_SHAPE (-3)   /* even kernel shape (CalcSol.py:58), kernel larger than the pad, indices out of range */
#define PS_ERR_BAD_ARG (-4)
#define PS_ERR_UNSUPPORTED (-5) /* FFT length not plannable (prime factor > 1024 or length > LDS) */
#define PS_ERR_HIP (-6)         /* HIP runtime error                                 */
#define PS_ERR_HPROB_BOUNDS (-7)/* ParasitoidModel.py:528-537  hprob out of bounds   */
#define PS_ERR_PMF_NEGATIVE (-8)/* ParasitoidModel.py:570,:589 pmf.min() < -1e-8     */
#define PS_ERR_FLIGHT_PROB (-9) /* ParasitoidModel.py:569,:571,:590 flight prob > 1 / negative loss */
#define PS_ERR_STATE (-10)      /* call order (e.g. fetch before run)                */
#define PS_ERR_EMPTY (-11)      /* prob_mass produced no entry >= 1e-8               */

#define PS_MODE_EXACT 0 /* FFT on the reference's torus P = N + K//2 (CalcSol.py:20-21) */
#define PS_MODE_FAST 1  /* FFT on the next even 7-smooth size >= P                       */
#define PS_MODE_FOLD 2  /* the reference's torus P, computed as a linear convolution on a fast
                         * FFT size >= P + K - 1 and folded back modulo P: exact-torus semantics
                         * at fast-size speed when P has large prime factors.  Chain API only
                         * (set_state, set_kernels, chain_run, records); the per-call
                         * fftconv2 / get_cursol / back_solve / spectrum calls return
                         * PS_ERR_UNSUPPORTED. */
#define PS_MODE_AUTO 3  /* exact reference-torus results by the cheapest route, chain API only: the
                         * day chain runs on the PS_MODE_FAST torus for as long as nothing above
                         * 1e-15 lies outside the N x N domain (then the two tori cannot differ by
                         * more than that per day: the pad holds no dust to wrap around).  Past
                         * that prefix, days that start from a domain-supported field and end
                         * flagged (largest value outside the domain > 1e-8) or clean run on a
                         * fast torus sized N + 2M, where they are true linear convolutions; the
                         * days in between -- sub-threshold dust the reference carries around its
                         * torus -- run as PS_MODE_FOLD.  ps_solver_auto_route tells which. */

typedef struct ps_solver ps_solver;
typedef struct ps_model ps_model;

typedef struct ps_day_stats {
  int64_t nnz;   /* entries with value*scale >= negval (r_small_vals, CalcSol.py:126-132) */
  double sum;    /* their sum                                                            */
  double delta;  /* (1-sum)/nnz added to every entry when renorm (CalcSol.py:134-135)    */
  double padmax; /* max over the pad region, clamped at 0 (CalcSol.py:36-37)             */
  int32_t flag;  /* padmax > 1e-8 -> state was truncated and re-transformed (:38,:200-201) */
  int32_t pad_;
} ps_day_stats;

/* ---- library ---------------------------------------------------------------- */
int ps_version(void);
int ps_device_count(void);             /* < 0 on error */
const char* ps_last_error(void);
/* device properties for reports: name[<=n], CU count, total HBM bytes */
int ps_device_info(int device, char* name, int n, int* cus, int64_t* hbm_bytes);
/* The unit list of the persistent forward row pass over kernel batches (no device needed): on a torus
 * of P rows whose day kernels wrap around row 0 with centre M (source row s sits at torus row
 * (s - M) mod P), a unit is np consecutive row pairs and is live when one of its rows holds a source
 * row of its entry's inclusive range ranges[2 d] .. ranges[2 d + 1] (empty when lo > hi).  Writes entry
 * and unit index of the first `cap` live units in list order; returns their total number, < 0 on
 * bad arguments. */
int ps_row_live_units(int P, int M, int np, int nd, const int32_t* ranges, int32_t* day, int32_t* unit, int cap);
/* Row pairs per workgroup (np) of the register-resident forward row kernels at FFT size fft_len, and whether
 * kernel batches of the full-column pipeline go to the persistent kernel there (no device needed); < 0 when
 * the size has no register-resident kernels. */
int ps_row_fwd_info(int fft_len, int* np, int* persistent);
/* Whether kernel batches with K x K boxes can go to the STAGED persistent kernel at FFT size fft_len (the next
 * unit's source rows copied to LDS while one is transformed; option PS_FWD_STAGE, off by default): its exchange
 * buffers and 2 np rows of K doubles in whole 1 KB chunks must fit in 160 KB together, else the plain
 * persistent kernel runs (no device needed);
 * < 0 when the size has no register-resident kernels.  ps_row_fwd_stage_lds: that kernel's LDS bytes (0: the
 * size keeps the one-shot kernel); ps_row_fwd_stage_bytes: the staged rows' share for np row pairs. */
int ps_row_fwd_stage_info(int fft_len, int K, int* staged);
int64_t ps_row_fwd_stage_lds(int fft_len, int K);
int64_t ps_row_fwd_stage_bytes(int np, int K);
/* The staging layout, for tests (no device needed).  slot: the double of the staging area that holds source
 * column col of staged row r when the source row starts at parity e (address / 8 mod 2); walk: the copy of
 * source row `row` of a 16-byte aligned buffer of rows x K doubles (K odd) into staged row r of nstaged --
 * image[slot] = index of the source element the copy puts there (untouched where it writes nothing). */
int ps_row_fwd_stage_slot(int K, int r, int e, int col);
int ps_row_fwd_stage_walk(int K, int64_t rows, int64_t row, int r, int nstaged, int64_t* image);

/* ---- solver: replaces class cuda_lib.CudaSolve (cuda_lib.py:16-221) and the
 *      CPU primitives CalcSol.fft2/fftconv2/ifft2/back_solve (CalcSol.py:11-109) */

/* CudaSolve.__init__ shape logic (cuda_lib.py:26-28): pad = dom_len + max_shape//2. */
int ps_solver_create(ps_solver** out, int device, int dom_len, int max_shape, int mode);
/* FFT size a PS_MODE_FAST solver would use for this domain and kernel shape (no device needed):
 * lets a caller size max_shape so that one solver serves a range of kernel shapes. */
int ps_fast_size(int dom_len, int max_shape);
/* PS_MODE_FOLD only: change the kernel shape limit (and with it the reference torus
 * P = N + max_shape/2) of an existing solver, keeping its FFT size, plans and buffers -- valid
 * while N + 3 (max_shape/2) fits the solver's FFT size (ps_solver_info).  The state has to be
 * set again afterwards. */
int ps_solver_retarget(ps_solver* s, int max_shape);
int ps_solver_destroy(ps_solver* s);
/* P = reference torus, Pfft = transform size in use, H = Pfft/2+1 */
int ps_solver_info(ps_solver* s, int* dom_len, int* P, int* Pfft, int* H);
/* Everything enqueued on the handle's stream is done and the last ps_chain_run is final (its last
 * window of days verified, see ps_chain_run) when this returns. */
int ps_solver_sync(ps_solver* s);
/* Tuning / A-B knobs.  The reference has one switch (globalvars.py:5: `cuda`); this library's
 * knobs (csrc/ps_config.h) exist for measurements and for the A/B legs of
 * the bit-identity tests.  Their names are those of the environment variables that seed them: the
 * environment is read once, when a handle is created, and never again -- afterwards a knob of a
 * live handle is changed with these calls (an auto-mode front passes it on to its helpers).
 * Creation-time knobs (register-resident kernels on/off, column split, chunk size ...) are refused
 * with PS_ERR_STATE, unknown names with PS_ERR_BAD_ARG. */
int ps_solver_set_option(ps_solver* s, const char* key, double value);
int ps_solver_get_option(ps_solver* s, const char* key, double* value);
/* measurement aid: 1 when the day kernels of the last transformed chunk were compact enough
 * for the direct-sum first column sub-pass inside the fused kernel (no separate launch) */
int ps_solver_kernels_direct(ps_solver* s);
/* measurement aid: 1 when the solver runs the full-column pipeline (column-major spectra, one
 * pass per column transform: register-resident FFT sizes in PS_MODE_FAST), 0 for the tiled
 * two-sub-pass column kernels */
int ps_solver_pipeline(ps_solver* s);
/* measurement aid, read-only (makes no run final): *pending = 1 while the last ps_chain_run's final window
 * is still unchecked (see ps_chain_run); counts[4] = runs that returned with a check pending, pending checks
 * that found a flag and redid the days behind it, runs whose kernel staging was queued ahead of that check,
 * host uploads that went through the handle's pinned staging.  Either pointer may be null. */
int ps_solver_deferred_info(ps_solver* s, int* pending, int64_t* counts);
/* PS_MODE_AUTO: *first_fold_day = first chain day of the last ps_chain_run that ran on the folded
 * reference torus (-1: every day was clean and ran on the fast torus); *fold_fft = FFT size of the
 * fold path (0 if it was never needed).  Other modes: -1 / 0. */
int ps_solver_auto_info(ps_solver* s, int* first_fold_day, int* fold_fft);
/* PS_MODE_AUTO: which solver produced each day [first, first+count) of the last ps_chain_run:
 * 0 the fast-torus front (clean prefix), 1 the wide fast-torus helper (N + 2M: flagged and clean
 * days past the prefix), 2 the fold child (days whose sub-threshold dust the reference carries),
 * 3 the narrow fast-torus helper (N + M, like the front: days a previous run saw flagged above 4e-8,
 * which makes the reference's flag certain on any torus). */
int ps_solver_auto_route(ps_solver* s, int first, int count, int32_t* owner);

/* CudaSolve.__init__ (cuda_lib.py:34-54) / CalcSol.fft2 (CalcSol.py:11-24):
 * state_hat = FFT2(zero-padded N x N sparse field).  The arrays are the caller's again when the
 * call returns: they are copied into pinned staging owned by the handle (grown on demand) and the
 * call enqueues without waiting for the stream.  Only if that pinned block cannot be allocated does
 * the call copy from the caller's arrays and wait for the stream instead. */
int ps_solver_set_state_coo(ps_solver* s, const int32_t* row, const int32_t* col,
                            const double* val, int64_t nnz);

/* CudaSolve.fftconv2 (cuda_lib.py:58-94) / CalcSol.fftconv2 (CalcSol.py:45-66):
 * wrap the odd kshape x kshape kernel to the origin, FFT, state_hat *= B_hat. */
int ps_solver_fftconv2_coo(ps_solver* s, const int32_t* row, const int32_t* col,
                           const double* val, int64_t nnz, int kshape);

/* CudaSolve.get_cursol (cuda_lib.py:98-140) / CalcSol.ifft2 (+ re-FFT, CalcSol.py:28-41,
 * :200-201): inverse transform, boundary flag, truncate + re-transform when flagged.
 * The N x N field stays on the device as chain record 0.  Statistics are taken on
 * value*stat_scale >= negval; renorm != 0 computes the prob-model delta. */
int ps_solver_get_cursol(ps_solver* s, double negval, double stat_scale, int renorm,
                         ps_day_stats* stats);

/* CudaSolve.back_solve (cuda_lib.py:145-221) / CalcSol.back_solve (CalcSol.py:72-109):
 * nfilt N x N filters in chronological order, concatenated COO with offsets
 * off[nfilt+1].  Results stay on the device as back-solve records 0..nfilt-1 in
 * emergence order; stats[nfilt] optional. */
int ps_solver_back_solve(ps_solver* s, int nfilt, const int64_t* off, const int32_t* row,
                         const int32_t* col, const double* val, double negval,
                         double stat_scale, ps_day_stats* stats);

/* ---- whole day chain: replaces the loops of CalcSol.get_solutions
 *      (CalcSol.py:191-201) and CalcSol.get_populations (:308-323, r_dur == 1) ---- */

/* Upload nk day kernels (pmf_list entries, ParasitoidModel.prob_mass output): COO
 * concatenated with offsets off[nk+1]; kshape[d] odd.  All kernel transforms are
 * batched up front (they do not depend on the state). */
int ps_chain_set_kernels(ps_solver* s, int nk, const int64_t* off, const int32_t* kshape,
                         const int32_t* row, const int32_t* col, const double* val);
/* Run days [first, first+count) from the current state: per day
 * fftconv2 -> ifft2 -> statistics/flag -> (flagged) truncate + re-FFT, all enqueued on
 * the handle's stream.  The flag decisions are taken on the device; the call itself waits for
 * the device only where it verifies a window of days that it ran without the conditional
 * launches.  A PS_MODE_FAST run on the full-column pipeline may return with its LAST window enqueued
 * but not yet verified: the library verifies it -- and redoes the days behind a flag, exactly as
 * the call itself would have -- at the start of the next call on the handle that reads or changes
 * anything of the run (statistics, records, profiling counters, kernels, options, another run,
 * ps_solver_sync, ...), so every result a caller can see is final.  ps_solver_set_state_* alone does
 * not: a sampler chain's set_state + ps_chain_run on the same kernels keeps the device busy across
 * the boundary.  Synchronising the device by other means (hipDeviceSynchronize) therefore does not
 * make a run final; ps_solver_sync does.  PS_NO_DEFER_CHECK=1: the call returns with the last window
 * verified.  Day d's field is chain record d; the
 * statistics of every day run since the kernels were uploaded stay readable (ps_chain_stats).
 * A run may be continued (first > 0 right after a run that ended at first) in PS_MODE_EXACT / FAST /
 * FOLD.  PS_MODE_AUTO runs need a fresh state (ps_solver_set_state_*) before EVERY call: once a run
 * has handed days over to its helpers the front solver's spectrum is void, and whether that happened
 * depends on the data (PS_ERR_STATE "auto mode: set the state before every chain run" otherwise). */
int ps_chain_run(ps_solver* s, int first, int count, double negval, double stat_scale,
                 int renorm);
int ps_chain_stats(ps_solver* s, int first, int count, ps_day_stats* out); /* synchronises */

/* get_populations with a multi-day release, r_dur > 1 (CalcSol.py:296-323; CudaSolve.back_solve,
 * cuda_lib.py:145-221, with its re-FFT semantics :208-214) on the chain API.  The LAST `nfilt`
 * entries of the uploaded kernel list are the release days' spreads r_spread[0 .. nfilt-1] in
 * chronological order, each cut to its support box about the centre (an odd kernel; it lands on the
 * torus where the reference wraps the N x N filter, CalcSol.py:86-91); the entries before them are
 * the day kernels.
 *   count > 0: for each day d of [first, first+count): the last cohort moves one day on (state *=
 *     K_d, inverse, truncate + re-transform on its flag), the back-solve runs through filters
 *     nuse-1 .. 0 from a copy of the state's spectrum, and the population
 *     sum_{i<nuse} weights[i] back_i + weights[nuse] cohort  becomes chain record d (its statistics:
 *     ps_chain_stats, scale 1, no renormalisation).
 *   count == 0: the back-solve alone from the state as it stands (a release day, CalcSol.py:298-306):
 *     sum_{i<nuse} weights[i] back_i + weights[nuse] state  ->  record (3, 0).
 * Enqueued without a host round trip per day.  *certified (may be NULL): PS_MODE_AUTO -- 1 when no
 * field of the run had anything above 1e-15 outside the domain, so the fast torus held what the
 * reference's torus holds (<= 4e-15 per day); 0: redo the run in PS_MODE_EXACT.  Other modes: 1.
 * PS_MODE_FOLD: PS_ERR_UNSUPPORTED. */
int ps_chain_run_release(ps_solver* s, int first, int count, double negval, int nfilt, int nuse,
                         const double* weights, int* certified);

/* One simulation split over G GPUs by days -- SURVEY.md 8e, the flag-free special case (the reference has no
 * counterpart: CalcSol.py:140-201 is one sequential loop; while no day raises its boundary flag that loop is the
 * product A_d = A_0 K_1 ... K_d of spectra, and products re-associate).  Every rank holds the same state and
 * the kernels of (at least) its own days.
 *   ps_chain_block_prefix: the running products L_i = K_first ... K_{first+i} of days [first, first+count)
 *     (2-D spectra in the solver's own layout, kept in the solver); *total_dev = device pointer of the block
 *     total L_{count-1}, *total_bytes its size -- valid until the next block call on s.  The ranks exchange
 *     these (one all-gather; parasitoids_amd/parallel.py:chain_prefix_split).
 *   ps_chain_block_finish: chain records and statistics of the same days from A_0 T_0 ... T_{nprev-1} L_i
 *     (prev_totals: device pointers of the nprev EARLIER blocks' totals, in block order, on this device; same
 *     layout, i.e. solvers of the same dom_len / max_shape); negval / stat_scale / renorm as ps_chain_run;
 *     *flagged = 1 when one of these days raised the flag -- the split does not apply then, rerun with
 *     ps_chain_run.  The state afterwards is the spectrum after the block's last day.
 * Same transforms and epilogue as ps_chain_run, the spectral products in another order: a field differs from
 * the sequential chain's by rounding only (tests/test_prefix_split_gpu.py: tested at <= 1e-14 of the
 * day's maximum over 12 days in up to 5 blocks, measured 1e-19 absolute on the 30-day headline stack in 8).  PS_MODE_FAST on a register-resident FFT size (PS_ERR_UNSUPPORTED otherwise). */
int ps_chain_block_prefix(ps_solver* s, int first, int count, const void** total_dev, int64_t* total_bytes);
int ps_chain_block_finish(ps_solver* s, int first, int count, int nprev, const void* const* prev_totals,
                          double negval, double stat_scale, int renorm, int* flagged);
/* device-to-device copy between a buffer of this library and a caller's (e.g. a tensor of the collective) */
int ps_device_copy(void* dst, const void* src, int64_t bytes);

/* ---- records (device-resident N x N fields) ----
 * kind 0: chain/get_cursol records, 1: back_solve records, 2: state (first day),
 * 3: scratch result of ps_weighted_sum. */
#define PS_REC_CHAIN 0
#define PS_REC_BACK 1
#define PS_REC_STATE 2
#define PS_REC_WSUM 3
/* (re)compute statistics of any record with the given threshold/scale */
int ps_record_stats(ps_solver* s, int kind, int idx, double negval, double stat_scale,
                    int renorm, ps_day_stats* out);
/* r_small_vals + coo_matrix(dense) order (CalcSol.py:112-136): entries with
 * v*stat_scale >= negval, row-major; value = (v*stat_scale + delta) * post_scale.
 * cap must be >= the nnz reported by the matching stats call. */
int ps_record_fetch_coo(ps_solver* s, int kind, int idx, double negval, double stat_scale,
                        double delta, double post_scale, int32_t* row, int32_t* col,
                        double* val, int64_t cap, int64_t* nnz_out);
/* The same entries as CSR triplets (indptr[N+1], indices, data): what `.tocsr()` of the COO
 * result holds and what the reference's result files store per day (Run.py:490-516,
 * read back by Plot_Result.py:511-524) -- straight from the device compaction, no host sort. */
int ps_record_fetch_csr(ps_solver* s, int kind, int idx, double negval, double stat_scale,
                        double delta, double post_scale, int32_t* indptr /* N+1 */,
                        int32_t* indices, double* data, int64_t cap, int64_t* nnz_out);
int ps_record_fetch_dense(ps_solver* s, int kind, int idx, double* out /* N*N */);
/* Point gather from a record: out[i] = v*scale at (rows[i], cols[i]), 0 where v*scale < negval
 * -- what indexing the thresholded daily CSR solutions returns in Bayes_funcs.popdensity_grid /
 * popdensity_to_emergence (Bayes_funcs.py:20-179), without shipping the field to the host. */
int ps_record_gather(ps_solver* s, int kind, int idx, int64_t n, const int32_t* rows,
                     const int32_t* cols, double scale, double negval, double* out);
/* The same cells from nrec records in one launch and one transfer: out[r * n + i].
 * popdensity_to_emergence reads the same field cells on every day between release and
 * collection (Bayes_funcs.py:60-118): one call per collection instead of one per day. */
int ps_record_gather_multi(ps_solver* s, int nrec, const int32_t* kind, const int32_t* idx, int64_t n,
                           const int32_t* rows, const int32_t* cols, double scale, double negval,
                           double* out);
/* sum_d w[d] * record(kind[d], idx[d]) -> record (PS_REC_WSUM,0)  (CalcSol.py:322) */
int ps_weighted_sum(ps_solver* s, int n, const int32_t* kind, const int32_t* idx,
                    const double* w);

/* ---- measurement: HIP-event timing per kernel class on the handle's stream ----
 * classes: 0 row_fwd, 1 col_fwd (first/single pass), 2 col_fwd (second sub-pass),
 * 3 col_inv (first pass, fused spectral product), 4 col_inv (second), 5 row_inv+epilogue,
 * 6 the three predicated passes of the flag-conditional re-FFT (no-ops when the flag is clear),
 * 7/8/9 class 3 for 2/4/8 consecutive days in one launch,
 * 10/11/12 class 5 for the 2/4/8 days of a chained group in one launch (full-column pipeline),
 * 13/14 classes 3/5 for any other number of days per launch (up to 32; a solver whose previous run
 *       raised no flag opens with such windows) -- ps_prof_read_days gives the grid-days they covered,
 * 15 the three short launches for the columns taken out of a chained pass (its thin last round) */
#define PS_PROF_NCLS 16
int ps_prof_enable(ps_solver* s, int on);   /* 0 off, 1 every launch, n > 1 every n-th launch per class */
int ps_prof_read(ps_solver* s, int ncls, double* total_ms, int64_t* count); /* synchronises */
int ps_prof_read_days(ps_solver* s, int ncls, int64_t* days); /* grid-days of the timed launches per class */
int ps_prof_read_launches(ps_solver* s, int ncls, int64_t* launches); /* ALL launches per class since ps_prof_enable (timed or not) */
/* the same four arrays for one owner of an auto-mode run: 0 the front itself, 1 wide, 2 fold child, 3 narrow
 * (the numbering of ps_solver_auto_route).  ps_prof_enable on the front switches its helpers too, helpers
 * attached later inherit it; a helper the run never needed reads as zeros. */
int ps_prof_read_owner(ps_solver* s, int owner, int ncls, double* total_ms, int64_t* count, int64_t* launches,
                       int64_t* days);
int ps_solver_owner_fft(ps_solver* s, int owner); /* torus size of that owner, 0 while it does not exist */

/* full P x P complex spectrum in/out (function-level CalcSol.fft2/fftconv2/ifft2 mirrors;
 * only valid in PS_MODE_EXACT) */
int ps_solver_get_spectrum(ps_solver* s, double* out /* P*P*2 */);
int ps_solver_set_spectrum(ps_solver* s, const double* in /* P*P*2 */);

/* ---- per-day kernel construction: replaces ParasitoidModel.prob_mass
 *      (ParasitoidModel.py:384-613) incl. h_flight_prob (:282-309) and
 *      get_mvn_cdf_values (:311-380) ---- */
int ps_model_create(ps_model** out, int device);
int ps_model_destroy(ps_model* m);
/* "PS_PM_SEG" (periods summed per prob_mass record, 8) and "PS_PM_SYNC" (1: never size the pair
 * lists from the previous batch); see ps_solver_set_option */
int ps_model_set_option(ps_model* m, const char* key, double value);
/* wind: float64 [ndays_wind][T][3] (windx, windy, windr), rows in the order of the
 * sorted day keys; day_keys[ndays_wind] the integer keys (prob_mass looks up day+1).
 * T == 1 rows with test_run != 0 reproduce the single-period mode (:422-428). */
int ps_model_set_wind(ps_model* m, const double* wind, const int32_t* day_keys, int ndays_wind,
                      int T, int test_run);
/* Build the kernels of nd days in one batch.  day_idx[i] indexes the wind rows;
 * start_time[i] < 0 means None.  hparams = (lam,aw,bw,a1,b1,a2,b2), Dparams/Dlparams =
 * (sig_x,sig_y,rho).  Outputs per day: kshape (odd side of the shrunk kernel), nnz,
 * warned (1 if a period left the domain, ParasitoidModel.py:549-557), status
 * (PS_OK or the assertion class that fired). */
int ps_model_prob_mass(ps_model* m, int nd, const int32_t* day_idx, const double* start_time,
                       const double* hparams, const double* Dparams, const double* Dlparams,
                       double mu_r, int n_periods, double rad_dist, int rad_res,
                       int32_t* kshape, int64_t* nnz, int32_t* warned, int32_t* status);
int ps_model_fetch_coo(ps_model* m, int i, int32_t* row, int32_t* col, double* val, int64_t cap);
/* diagnostics for tests: hprob[T] of day i of the last batch, stamp half-widths H[T] */
int ps_model_fetch_debug(ps_model* m, int i, double* hprob, int32_t* Hs, double* loss,
                         double* pmfsum);
/* h_flight_prob (ParasitoidModel.py:282-309) of wind row day_i: out[T] */
int ps_model_hflight(ps_model* m, int day_i, const double* hparams, double* out);
/* get_mvn_cdf_values (ParasitoidModel.py:311-380) for one (cell, mu, S): returns the
 * half width; fills out[(2H+1)^2] when cap allows. */
int ps_model_mvn_cdf_values(ps_model* m, double cell, double mu_x, double mu_y, double sig_x,
                            double sig_y, double rho, int32_t* H, double* out, int64_t cap);
/* hand the kernels of the last batch straight to a solver on the same device
 * (no host round trip): equivalent to ps_chain_set_kernels with days [first, first+count). */
int ps_chain_set_kernels_from_model(ps_solver* s, ps_model* m, int first, int count);
/* The same with kernels idx[0..count) of the last batch, in that order, repeats allowed: equivalent to
 * ps_chain_set_kernels with those kernels, so that many sequences of days run over one batch (weather
 * ensembles).  One launch (k_gather_kernels: one block row per kernel, grid-stride over its entries) copies the
 * chosen segments of the model's COO pool into a staging block the model owns, on the model's stream; the
 * solver's stream waits for it by event and copies the block, and the next gather waits for that copy: no host
 * synchronisation of its own.  PS_ERR_BAD_ARG: a null handle, count < 0, a null idx with count > 0, more than
 * 65535 kernels, solver and model on different devices; PS_ERR_STATE: an index outside the last batch; a failed
 * day's own status. */
int ps_chain_set_kernels_from_model_indexed(ps_solver* s, ps_model* m, const int32_t* idx, int count);
int ps_solver_set_state_from_model(ps_solver* s, ps_model* m, int i);

/* ---- device-resident exchange between ranks (Run.py:412-425 maps prob_mass over a process pool; here
 * the days are sharded over the GPUs of a node and the COO kernels all-gathered with RCCL over xGMI).
 * The library does not know the communicator: the caller owns the device buffers of the collective and
 * passes raw DEVICE pointers (the only entry points that take device memory from outside).
 *   ps_model_export_device      concatenated triplets (int32 row, int32 col, float64 val) of days
 *                               [first, first+count) of the last batch -> caller's buffers (cap entries)
 *   ps_chain_set_kernels_device ps_chain_set_kernels from device triplets (copied before return)
 *   ps_solver_set_state_device  ps_solver_set_state_coo from the device triplets of an odd
 *                               kshape x kshape kernel, re-centred into the domain (Run.py:454-458) */
int ps_model_export_device(ps_model* m, int first, int count, void* row_dev, void* col_dev, void* val_dev,
                           int64_t cap);
int ps_chain_set_kernels_device(ps_solver* s, int nk, const int64_t* off, const int32_t* kshape,
                                const void* row_dev, const void* col_dev, const void* val_dev);
int ps_solver_set_state_device(ps_solver* s, const void* row_dev, const void* col_dev, const void* val_dev,
                               int64_t nnz, int kshape);

/* ---- posterior predictive spread: per-cell weighted moments of many model evaluations ----
 * (no reference counterpart: CompareToData.assess_fit / Plot_Result show one run at a point estimate).
 * A summary lives on one device and holds nslot day slots of N x N cells; per cell the weighted mean and
 * M2 (fp64) and one uint32 count per threshold (0..4): the weight of the members whose value reached it.
 * Host side: the total weight W (< 2^32: the counts are exact) and the member count.  One thread owns a
 * cell: no atomics, the result is bitwise the same for the same members in the same order. */
typedef struct ps_summary ps_summary;
/* thr[nthr] thresholds (v >= thr counts) */
int ps_summary_create(int device, int N, int nslot, int nthr, const double* thr, ps_summary** out);
/* Accumulate one member with integer weight w >= 1 from the records of solver s (same device, same N):
 * slot i reads record (kind[i], idx[i]) and adds, per cell, exactly what the matching
 * ps_record_fetch_* returns there (0 where it returns no entry):
 *   t = rec * stat_scale[i];  v = (t != 0 && !(t < negval)) ? (t + delta) * post_scale[i] : 0
 * delta = the day's device statistics' delta when use_delta[i] (chain records), else 0.  Weighted Welford
 * (West 1979): W' = W + w, d = v - mean, mean += d w / W', M2 += w d (v - mean).  One launch on the
 * solver's stream, no host synchronisation; an event orders it after the summary's previous operation
 * on whatever stream that ran.  nslot must equal the summary's. */
int ps_summary_add(ps_summary* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                   const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                   double negval, uint32_t weight);
/* dst += src (Chan et al. pairwise update), same device, N, slots and thresholds; src stays as it is */
int ps_summary_merge(ps_summary* dst, ps_summary* src);
int ps_summary_info(ps_summary* a, double* total_weight, int64_t* members);
/* one slot to the host (synchronises): what 0 mean, 1 variance M2 / W, 2 + k P(v >= thr[k]) = count_k / W.
 * PS_ERR_STATE at W = 0. */
int ps_summary_fetch(ps_summary* a, int slot, int what, double* out /* N*N */);
int ps_summary_reset(ps_summary* a);
/* measurement: HIP-event timing of the ps_summary_add launches.  enable 1 on, 0 off, < 0 unchanged;
 * total_ms / launches (either may be NULL) receive the timed launches since creation (synchronises).
 * Every ps_*_prof of an accumulator or fields handle below works alike: while enabled a launch keeps one
 * event pair; finished pairs are folded into running totals and their events destroyed on every read and,
 * with one host synchronisation, once 256 are pending on a channel, so a profiled handle holds a bounded
 * number of events however long it lives.  Nothing of this runs while profiling is off. */
int ps_summary_prof(ps_summary* a, int enable, double* total_ms, int64_t* launches);
void ps_summary_destroy(ps_summary* a);

/* ---- linearised spread: delta-method maps around a point estimate ----
 * The spread map of the normal approximation that Bayes_MAP.py:525 fits (pymc.NormApprox: MAP + the
 * inverse Hessian of the joint log density); the reference reports only the parameter covariance.
 * A handle lives on one device and holds nslot day slots of N x N cells (pitch = N*N rounded up to 64),
 * all fp64: center[slot], J[param][slot] (per-cell sensitivities dU/dtheta_i), and after finalisation
 * var[slot] and exc[k][slot].  Limits: nparam <= 16, nthr <= 4.  The whole block,
 * (nparam + 2 + nthr) * nslot * pitch * 8 bytes, is checked against the free device memory first:
 * PS_ERR_OOM before anything is allocated.  One thread owns a pair of cells: no atomics, the same calls
 * in the same order give the same bits.  Every operation records an event that the next one waits on,
 * on whatever stream it runs (the solver's for set_center / add, the handle's own otherwise). */
typedef struct ps_linspread ps_linspread;
/* thr[nthr] thresholds (exceedance P(U >= thr)) */
int ps_linspread_create(int device, int N, int nslot, int nparam, int nthr, const double* thr, ps_linspread** out);
/* center[slot i] = the value record (kind[i], idx[i]) of solver s holds at each cell, by the rule of
 * ps_summary_add (what ps_record_fetch_* returns there, 0 where it returns no entry):
 *   t = rec * stat_scale[i];  v = (t != 0 && !(t < negval)) ? (t + delta) * post_scale[i] : 0
 * One launch on the solver's stream, no host synchronisation. */
int ps_linspread_set_center(ps_linspread* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                            double negval);
/* J[param][slot i] += coef * v (v as above) for every slot in one launch on the solver's stream; cell
 * pairs whose values are both 0 are not stored.  A central difference over a stencil pair:
 * add(i, +1/(2h), at theta + h e_i), add(i, -1/(2h), at theta - h e_i).  coef finite and non-zero. */
int ps_linspread_add(ps_linspread* h, ps_solver* s, int param, double coef, int nslot, const int32_t* kind,
                     const int32_t* idx, const double* stat_scale, const double* post_scale,
                     const int32_t* use_delta, double negval);
/* Sigma = F F' (F: nparam x rank, row-major, rank <= 16; nparam must equal the handle's).  Per cell
 *   var = sum_k (sum_i F_ik J_i)^2   (never negative, unlike J' Sigma J with round-off)
 *   exc_k = 0.5 erfc((thr_k - center) / (sqrt(var) sqrt 2)),  exactly (center >= thr_k) where var == 0.
 * PS_ERR_STATE without a centre.  Any later set_center / add invalidates the result. */
int ps_linspread_finalize(ps_linspread* h, int nparam, int rank, const double* F);
/* one slot to the host (synchronises): what 0 centre, 1 variance, 2 + k exceedance k, 16 + i J_i.
 * PS_ERR_STATE for the centre before set_center and for 1.. before finalize. */
int ps_linspread_fetch(ps_linspread* h, int slot, int what, double* out /* N*N */);
/* state: centre set, finalized, adds per parameter (adds[nparam]); any pointer may be NULL */
int ps_linspread_info(ps_linspread* h, int* centered, int* finalized, int64_t* adds);
int ps_linspread_reset(ps_linspread* h);
/* measurement: HIP-event timing of the add and finalize launches (not set_center).  enable 1 on, 0 off,
 * < 0 unchanged; the totals so far go to the non-NULL outputs (synchronises). */
int ps_linspread_prof(ps_linspread* h, int enable, double* add_ms, int64_t* add_launches, double* fin_ms,
                      int64_t* fin_launches);
void ps_linspread_destroy(ps_linspread* h);

/* ---- posterior predictive histograms: per-cell weighted distributions on fixed bin edges ----
 * (no reference counterpart).  A histogram lives on one device and holds nslot day slots of N x N cells
 * and a strictly increasing edge table e_0 < ... < e_B (2 <= nedge = B + 1 <= 1024, every edge finite
 * and > 0), uploaded once.  Bin b = searchsorted(edges, v, side='right'): bin 0 holds v < e_0 (zeros
 * included), bin b in 1..B holds e_{b-1} <= v < e_b, bin B + 1 holds v >= e_B.  Per slot uint32 count
 * planes [b = 1 .. B+1][pitch] (bin-major; bin 0 is W - the rest, never stored) and one word per cell with
 * its lowest and highest touched bin, so that quantiles and exceedances read only those planes.  The
 * full size, nslot * pitch * (nedge + 1) * 4 B, is checked against the free device memory first:
 * PS_ERR_OOM before anything is allocated.  Host side: W (< 2^32) and the member count.  Counts are
 * integers and one thread owns a pair of cells: no atomics, and neither the order of adds nor that of
 * merges changes a bit.  Every operation records an event the next one waits on, whichever stream it
 * runs on (the solver's for add, the handle's own otherwise). */
typedef struct ps_hist ps_hist;
int ps_hist_create(int device, int N, int nslot, int nedge, const double* edges, ps_hist** out);
/* count_b(v) += weight for every slot and cell, v by the rule of ps_summary_add (same arguments, same
 * value bit for bit).  One launch on the solver's stream, no host synchronisation. */
int ps_hist_add(ps_hist* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                uint32_t weight);
/* dst += src (counts add), same device, N, slots and edges; src stays as it is */
int ps_hist_merge(ps_hist* dst, ps_hist* src);
int ps_hist_info(ps_hist* h, double* total_weight, int64_t* members, int* nedge);
/* One slot's quantile at p in (0, 1] (synchronises; any output may be NULL).  C_b = the weight through
 * bin b, b* = the smallest b with (double)C_b >= p * (double)W.  lower / upper: the bracket
 * [e_{b*-1}, e_{b*}) that holds the exact weighted lower quantile, [0, e_0) at b* = 0, [e_B, inf) at
 * b* = B + 1.  value: e_{b*-1} * (e_{b*} / e_{b*-1})^f with f = (p W - C_{b*-1}) / count_{b*} for
 * 1 <= b* <= B, 0 at b* = 0, e_B at b* = B + 1.  PS_ERR_STATE at W = 0. */
int ps_hist_quantile(ps_hist* h, int slot, double p, double* value, double* lower, double* upper);
/* P(v >= e_k) = (W - C_k) / W per cell, exact (synchronises).  PS_ERR_STATE at W = 0. */
int ps_hist_exceed(ps_hist* h, int slot, int k, double* out /* N*N */);
/* count of bin b (0 .. B + 1) per cell; bin 0 derived as W - the rest (synchronises) */
int ps_hist_fetch_counts(ps_hist* h, int slot, int b, uint32_t* out /* N*N */);
int ps_hist_reset(ps_hist* h);
/* measurement: HIP-event timing of the add and quantile launches.  enable 1 on, 0 off, < 0 unchanged;
 * the totals so far go to the non-NULL outputs (synchronises). */
int ps_hist_prof(ps_hist* h, int enable, double* add_ms, int64_t* add_launches, double* q_ms,
                 int64_t* q_launches);
void ps_hist_destroy(ps_hist* h);

/* ---- posterior arrival maps: when the members reach each cell, and the area they reach ----
 * (no reference counterpart).  A handle lives on one device and holds nslot day slots (1..32) of N x N
 * cells and 1..4 strictly increasing thresholds t_0 < ... < t_{K-1}, each finite and > 0.  For one member,
 * v_s(c) is the value ps_summary_add adds for slot s (same arguments, same value bit for bit), and the
 * arrival slot is a_k(c) = min{s : v_s(c) >= t_k}, nslot ("never") if no slot qualifies.  Per threshold
 * and slot uint32 count planes cnt[k][s][pitch] (pitch as ps_summary): the weight of the members with
 * a_k(c) = s; "never" is W - the rest, not stored.  Per member, in add order, its reached cells
 * n_k(s) = #{c : a_k(c) <= s} and its weight; a merge appends src's members after dst's.  The whole count
 * block, nthr * nslot * pitch * 4 B plus scratch, is checked against the free device memory first:
 * PS_ERR_OOM before anything is allocated.  Host side: W (< 2^32) and the member count.  Counts are
 * integers and every cell has one writer: neither the order of adds, nor that of merges, nor the launch
 * configuration changes a bit.  Every operation records an event the next one waits on, whichever stream
 * it runs on (the solver's for add, the handle's own otherwise). */
typedef struct ps_arrival ps_arrival;
int ps_arrival_create(int device, int N, int nslot, int nthr, const double* thr, ps_arrival** out);
/* One member with weight >= 1 (arguments as ps_hist_add): one launch walks the slots of every cell pair in
 * order, a second small one sums the member's n_k(s), both on the solver's stream, no host synchronisation
 * (except once when the member rows double their capacity). */
int ps_arrival_add(ps_arrival* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                   const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                   uint32_t weight);
/* dst += src (counts add, src's member rows appended), same device, N, slots and thresholds; src unchanged */
int ps_arrival_merge(ps_arrival* dst, ps_arrival* src);
int ps_arrival_info(ps_arrival* a, double* total_weight, int64_t* members);
/* P(arrived by slot) = C_k[slot] / W per cell, C_k[s] = sum over s' <= s of the counts (synchronises).
 * PS_ERR_STATE at W = 0. */
int ps_arrival_prob(ps_arrival* a, int k, int slot, double* out /* N*N */);
/* the smallest slot s with (double)C_k[s] >= p * (double)W per cell, -1 where even the last slot falls
 * short; p in (0, 1] (synchronises).  PS_ERR_STATE at W = 0. */
int ps_arrival_quantile(ps_arrival* a, int k, double p, int32_t* out /* N*N */);
/* count plane of threshold k and slot 0 .. nslot; slot == nslot: never, W - the rest (synchronises) */
int ps_arrival_fetch_counts(ps_arrival* a, int k, int slot, uint32_t* out /* N*N */);
/* members first .. first + count - 1: cells[count][nthr][nslot] = n_k(s), weights[count] (either may be NULL;
 * synchronises) */
int ps_arrival_fetch_reached(ps_arrival* a, int64_t first, int64_t count, uint32_t* cells, uint32_t* weights);
int ps_arrival_reset(ps_arrival* a);
/* measurement: HIP-event timing of the add launches (both kernels) and of the map launches (prob, quantile,
 * never counts).  enable 1 on, 0 off, < 0 unchanged; the totals so far go to the non-NULL outputs
 * (synchronises). */
int ps_arrival_prof(ps_arrival* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps);
void ps_arrival_destroy(ps_arrival* a);

/* ---- projections over time: emergence and cumulative exposure of one member, as maps ----
 * (the map-level form of Bayes_funcs.popdensity_to_emergence, which projects at the observation cells only).
 * A handle lives on one device and holds a weight matrix W[nout][nin] (row-major, 1 <= nin <= 32 input
 * records, 1 <= nout <= 32 outputs, every weight finite and >= 0, no row all zeros: PS_ERR_BAD_ARG
 * otherwise), uploaded once at create, and nout fp64 output fields Y[e][pitch] (pitch as ps_summary).  For
 * one member, v_d(c) is the value ps_summary_add adds for input record d (same arguments, same value bit for
 * bit), and an apply overwrites every cell of every output with
 *   Y_e(c) = sum over d of W[e][d] * v_d(c)
 * summed from +0.0 in ascending d with the product and the sum rounded separately (acc = acc + w * v in
 * IEEE double, never fused); a zero weight changes no bit, so the numpy loop that skips zero weights gives
 * the same bits.  One thread owns a pair of cells and a tile of 8 outputs; a record is read once per tile
 * that has a non-zero weight for it.  No atomics: the same call gives the same bits.  The full size,
 * nout * pitch * 8 B plus the weight tables, is checked against the free device memory first: PS_ERR_OOM
 * before anything is allocated.  Every operation records an event the next one waits on, whichever stream
 * it runs on (the solver's for apply, the handle's own for fetch and gather, the accumulator's for
 * ps_summary_add_project and ps_hist_add_project). */
typedef struct ps_project ps_project;
int ps_project_create(int device, int N, int nin, int nout, const double* W /* nout x nin */, ps_project** out);
/* Project the records of solver s (same device, same N; arguments as ps_summary_add, nin must equal the
 * handle's): one launch on the solver's stream, no host synchronisation, nothing copied or allocated. */
int ps_project_apply(ps_project* p, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                     const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* one output field to the host (synchronises).  PS_ERR_STATE before the first apply. */
int ps_project_fetch(ps_project* p, int e, double* out /* N*N */);
/* the outputs at n listed cells: out[e * n + k] = Y_e(rows[k], cols[k]) (synchronises).  PS_ERR_BAD_ARG for
 * a cell outside the domain, PS_ERR_STATE before the first apply. */
int ps_project_gather(ps_project* p, int64_t n, const int32_t* rows, const int32_t* cols, double* out /* nout x n */);
/* any pointer may be NULL */
int ps_project_info(ps_project* p, int* N, int* nin, int* nout, int64_t* applies);
/* measurement: HIP-event timing of the apply launches.  enable 1 on, 0 off, < 0 unchanged; total_ms /
 * launches (either may be NULL) receive the timed launches so far (synchronises). */
int ps_project_prof(ps_project* p, int enable, double* total_ms, int64_t* launches);
void ps_project_destroy(ps_project* p);
/* One member with weight >= 1 whose values are the projection's current outputs: slot e of the accumulator
 * takes Y_e, through the accumulator's own add kernel and update rule (ps_summary_add / ps_hist_add), on the
 * accumulator's stream behind the projection's last operation; the projection's next apply waits for it.
 * The accumulator's slot count must equal the projection's nout, device and N must agree (PS_ERR_BAD_ARG,
 * nothing enqueued); PS_ERR_STATE before the projection's first apply.  Weight and members advance as in add. */
int ps_summary_add_project(ps_summary* a, ps_project* p, uint32_t weight);
int ps_hist_add_project(ps_hist* h, ps_project* p, uint32_t weight);
/* The same for arrival maps: slot e of the handle takes Y_e, so the slots are the projection's outputs in
 * ascending order (nslot must equal nout) and a member's arrival slot is the first output that reaches the
 * threshold.  Both kernels of an arrival add run on the handle's stream. */
int ps_arrival_add_project(ps_arrival* a, ps_project* p, uint32_t weight);

/* ---- release plans: several release sites and staggered release days of one member, as maps ----
 * (no reference counterpart: the reference releases once, at the domain centre).  One wind station and a
 * homogeneous landscape make the field of a release at another cell the centre release translated, and the
 * population chain is linear in the released number.  A release `lag` days later is not a time shift (every
 * day has its own kernel): it is the run of a solver of its own over the later days.  A handle lives on one
 * device and holds the sites group by group -- a group is the set of sites that share one release day, so
 * one solver -- and nout fp64 output fields Y[e][pitch] (pitch as ps_summary):
 *   Y_e(r, c) = sum over the groups g and the sites k of g of amount_k * v_{g,e}(r - drow_k, c - dcol_k)
 * v_{g,e} the value ps_summary_add adds for the record that group g's apply names for output e (same
 * arguments, same value bit for bit), 0 where the source row or the source column lies outside [0, N): mass
 * that leaves the east edge does not come back at the west edge of the next row.  Limits: 1 <= nout <= 32,
 * 1 <= ngroup <= 8, every group_nsite >= 1, at most 32 sites in all, |drow|, |dcol| <= N - 1, every amount
 * finite and > 0; anything else is PS_ERR_BAD_ARG with the offender named.  drow, dcol and amount list the
 * sites of group 0, then those of group 1, and so on.  Arithmetic: per cell and output, acc starts from +0.0
 * in group 0 and from the stored Y in later groups, and takes the group's sites in the order given as
 * acc = acc + amount * v in IEEE double, product and sum rounded separately, never fused; a term from outside
 * the domain adds +0.0 to acc >= +0.0 and changes no bit.  Every cell has one writer, no atomics: the same
 * calls give the same bits.  nout * pitch * 8 B is checked against the free device memory first: PS_ERR_OOM
 * before anything is allocated.  Every operation records an event the next one waits on, whichever stream
 * it runs on (the group's solver's for apply, the handle's own for fetch and gather, the accumulator's for
 * the add entry points below), so the solvers of different groups may run on different streams. */
#define PS_REC_NONE (-1)   /* ps_sites_apply only: the group is not released yet on that output day */
typedef struct ps_sites ps_sites;
int ps_sites_create(int device, int N, int nout, int ngroup, const int32_t* group_nsite, const int32_t* drow,
                    const int32_t* dcol, const double* amount, ps_sites** out);
/* Apply group `group` from the records of solver s (same device, same N; nout must equal the handle's): slot e
 * names the record of model day D_e - lag_group of that solver (arguments as ps_summary_add), or has kind
 * PS_REC_NONE and contributes nothing; at least one slot must name a record.  One launch on the solver's
 * stream, no host synchronisation, nothing copied or allocated; every descriptor is resolved before anything
 * is enqueued.  The groups of a pass go in the order 0, 1, ..., ngroup - 1: group 0 overwrites Y, zeros
 * included, later groups accumulate; any other group is PS_ERR_STATE (group 0 alone may come early: it
 * abandons the pass under way and opens a new one).  A pass is complete once its last group is applied; fetch, gather and the add entry points are PS_ERR_STATE before the first complete pass
 * and while a pass is under way. */
int ps_sites_apply(ps_sites* p, ps_solver* s, int group, int nout, const int32_t* kind, const int32_t* idx,
                   const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* one output field to the host (synchronises) */
int ps_sites_fetch(ps_sites* p, int e, double* out /* N*N */);
/* the outputs at n listed cells: out[e * n + k] = Y_e(rows[k], cols[k]) (synchronises).  PS_ERR_BAD_ARG for a
 * cell outside the domain. */
int ps_sites_gather(ps_sites* p, int64_t n, const int32_t* rows, const int32_t* cols, double* out /* nout x n */);
/* any pointer may be NULL; passes: the complete passes so far */
int ps_sites_info(ps_sites* p, int* N, int* nout, int* ngroup, int* nsite, int64_t* passes);
/* measurement: HIP-event timing of the apply launches (one per group and pass).  enable 1 on, 0 off, < 0
 * unchanged; total_ms / launches (either may be NULL) receive the timed launches so far (synchronises). */
int ps_sites_prof(ps_sites* p, int enable, double* total_ms, int64_t* launches);
void ps_sites_destroy(ps_sites* p);
/* One member with weight >= 1 whose values are the plan's current outputs, as the add_project entry points
 * take a projection's: slot e of the accumulator takes Y_e, on the accumulator's stream behind the plan's
 * last apply; the plan's next apply waits for it.  Slot count, device and N must agree (PS_ERR_BAD_ARG,
 * nothing enqueued). */
int ps_summary_add_sites(ps_summary* a, ps_sites* p, uint32_t weight);
int ps_hist_add_sites(ps_hist* h, ps_sites* p, uint32_t weight);
int ps_arrival_add_sites(ps_arrival* a, ps_sites* p, uint32_t weight);

/* ---- posterior sensitivity maps: which scalar of the members drives the spread of each cell ----
 * (no reference counterpart; the global form of the J maps of ps_linspread, from the members of a chain
 * instead of a stencil around a point estimate).  A generic accumulator of the weighted co-moments between
 * fields and nparam scalars that the caller supplies per member -- the handle does not know what they are.
 * It lives on one device and holds nslot slots of N x N cells (pitch as ps_summary), all fp64: mean[slot],
 * M2[slot], C[param][slot] with C_i = sum over the members of w (v - mean_before) (theta_i - thetabar_i,after),
 * and after finalisation expl[slot] (fp64) and dom[slot] (uint8).  Limits: 1 <= nparam <= 16, nslot >= 1.
 * The whole block, ((nparam + 3) * 8 + 1) * nslot * pitch bytes, is checked against the free device memory
 * first: PS_ERR_OOM before anything is allocated.  Host side: the total weight W (< 2^32) and the member
 * count.  One thread owns a pair of cells: no atomics, the same calls in the same order give the same bits.
 * Every operation records an event that the next one waits on, on whatever stream it runs (the solver's for
 * add, the handle's own otherwise). */
typedef struct ps_sens ps_sens;
int ps_sens_create(int device, int N, int nslot, int nparam, ps_sens** out);
/* Accumulate one member with integer weight w >= 1 from the records of solver s: the slot descriptors and
 * the value v of a cell are those of ps_summary_add (same arguments, same value bit for bit).  e[nparam]:
 * the member's deviation of every scalar from that scalar's weighted mean AFTER this member, computed by
 * the caller; every e finite, nparam the handle's.  Per cell, with W' = W + w and d = v - mean:
 *   d == 0: nothing changes, nothing is stored; else
 *   mean += d w / W',  M2 += w d (v - mean)        (the statements of ps_summary_add: the same bits)
 *   C_i = C_i + (w d) e_i                          (w d, the product and the sum each rounded on its own)
 * so a host loop with one rounded operation per statement reproduces mean and every C_i bit for bit.  A pair
 * of cells with d == 0 in both reads the record and the two moments and touches no C_i.  One launch per 32
 * slots on the solver's stream, no host synchronisation; every descriptor is resolved before anything is
 * enqueued. */
int ps_sens_add(ps_sens* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                int nparam, const double* e, uint32_t weight);
/* The same member whose values are the current outputs of a projection or a release plan, as
 * ps_summary_add_project / ps_summary_add_sites take them: slot k takes Y_k, on the handle's stream behind the
 * source's last operation; its next apply waits for the read.  PS_ERR_STATE where the source has no finished
 * fields. */
int ps_sens_add_project(ps_sens* h, ps_project* p, int nparam, const double* e, uint32_t weight);
int ps_sens_add_sites(ps_sens* h, ps_sites* p, int nparam, const double* e, uint32_t weight);
/* dst += src (Chan et al. pairwise update), same device, N, slots and nparam; src stays as it is.
 * dtheta[i] = the weighted mean of scalar i over src's members minus that over dst's, from the caller:
 *   mean, M2 as ps_summary_merge;  C_i = Ca_i + Cb_i + (mean_b - mean_a) dtheta_i (Wa Wb / W).
 * Into an empty dst (W = 0) it is a device copy, bit for bit. */
int ps_sens_merge(ps_sens* dst, ps_sens* src, int nparam, const double* dtheta);
/* F: nparam x rank, row-major, rank <= 16, with F F' the (pseudo-)inverse of the scalars' covariance;
 * isd[nparam]: their inverse standard deviations (0 for a scalar to be left out).  Per cell, with
 * c_i = C_i / W and var = M2 / W, every product, sum and quotient rounded on its own, the sums from +0.0 in
 * ascending index:
 *   expl = (sum_k (sum_i F_ik c_i)^2) / var     the share of var a linear dependence on the scalars explains
 *                                               (a sum of squares: never negative; exactly 0 where M2 == 0)
 *   dom  = the lowest i that maximises (c_i isd_i)^2, compared by a strict > in index order
 *                                               (255 where M2 == 0 or every square is 0)
 * PS_ERR_STATE at W = 0.  Any later add, merge or reset invalidates the result. */
int ps_sens_finalize(ps_sens* h, int nparam, int rank, const double* F, const double* isd);
/* one slot to the host (synchronises): what 0 mean, 1 variance M2 / W, 2 expl, 3 dom as doubles (-1 for 255),
 * 16 + i covariance C_i / W.  PS_ERR_STATE at W = 0, and for 2 and 3 unless finalized since the last change. */
int ps_sens_fetch(ps_sens* h, int slot, int what, double* out /* N*N */);
int ps_sens_info(ps_sens* h, double* total_weight, int64_t* members);
int ps_sens_reset(ps_sens* h);
/* measurement: HIP-event timing of the add launches, as ps_summary_prof */
int ps_sens_prof(ps_sens* h, int enable, double* total_ms, int64_t* launches);
void ps_sens_destroy(ps_sens* h);

/* ---- posterior dependence maps: the correlation ratio of each cell on each scalar of the members ----
 * (no reference counterpart; where ps_sens measures a linear dependence, this measures any dependence of the
 * cell on ONE scalar at a time: eta2_p = Var_b(E[v | scalar p in bin b]) / Var(v), Pearson's correlation ratio,
 * the given-data estimator of the first-order variance-based index.)  A generic accumulator of per-bin sums
 * of fields: the caller bins every scalar of a member and passes the bin indices -- the handle does not know
 * what the scalars or the bin edges are.  It lives on one device and holds nslot slots of N x N cells (pitch
 * as ps_summary), all fp64: mean[slot], M2[slot], S[param][bin][slot] with S_pb = the sum of w v over the
 * members whose scalar p fell in bin b, and after finalisation eta[param][slot] (fp64) and dom[slot] (uint8).
 * Limits: 1 <= nparam <= 16, 2 <= nbin <= 16, nslot >= 1.  The whole block,
 * ((2 + nparam * nbin + nparam) * 8 + 1) * nslot * pitch bytes, is checked against the free device memory
 * first: PS_ERR_OOM before anything is allocated.  Host side: the total weight W (< 2^32) and the member
 * count.  One thread owns a pair of cells: no atomics, the same calls in the same order give the same bits.
 * Every operation records an event that the next one waits on, on whatever stream it runs (the solver's for
 * add, the handle's own otherwise). */
typedef struct ps_depend ps_depend;
int ps_depend_create(int device, int N, int nslot, int nparam, int nbin, ps_depend** out);
/* Accumulate one member with integer weight w >= 1 from the records of solver s: the slot descriptors and
 * the value v of a cell are those of ps_summary_add (same arguments, same value bit for bit).  bin[nparam]:
 * the member's bin of every scalar, each in 0..nbin - 1, nparam the handle's.  Per cell, with W' = W + w:
 *   d = v - mean;  where d != 0:  mean += d w / W',  M2 += w d (v - mean)
 *                                                  (the statements of ps_summary_add: the same bits)
 *   wv = w v;  S[p][bin[p]] = S[p][bin[p]] + wv    for every p (the product and the sum each rounded on its own)
 * so a host loop with one rounded operation per statement reproduces mean and every S plane bit for bit.  A
 * pair of cells with v == 0 in both reads the record and the two moments and touches no S.  One launch per 32
 * slots on the solver's stream, no host synchronisation; every descriptor is resolved before anything is
 * enqueued.  A bin out of range, a weight of 0, another nparam or nslot than the handle's, or a total weight
 * that would reach 2^32: PS_ERR_BAD_ARG, nothing is added anywhere. */
int ps_depend_add(ps_depend* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                  const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                  int nparam, const int32_t* bin, uint32_t weight);
/* The same member whose values are the current outputs of a projection or a release plan, as
 * ps_summary_add_project / ps_summary_add_sites take them: slot k takes Y_k, on the handle's stream behind the
 * source's last operation; its next apply waits for the read.  PS_ERR_STATE where the source has no finished
 * fields. */
int ps_depend_add_project(ps_depend* h, ps_project* p, int nparam, const int32_t* bin, uint32_t weight);
int ps_depend_add_sites(ps_depend* h, ps_sites* p, int nparam, const int32_t* bin, uint32_t weight);
/* dst += src, same device, N, slots, nparam and nbin (the caller answers for equal bin edges); src stays as it
 * is.  Every operation rounded on its own, in this order, W = Wa + Wb:
 *   fb = Wb / W;  fab = (Wa Wb) / W;  d = mean_b - mean_a
 *   mean = mean_a + d fb;  M2 = (M2_a + M2_b) + (d d) fab        (Chan et al., the formulas of ps_summary_merge)
 *   S_pb = S_pb,a + S_pb,b                                       plane by plane
 * Into an empty dst (W = 0) it is a device copy, bit for bit. */
int ps_depend_merge(ps_depend* dst, ps_depend* src);
/* Wb: nparam x nbin, row-major, the weight of the members per scalar and bin: integers in 0..2^32 - 1 held
 * exactly as doubles, every row summing to W (PS_ERR_BAD_ARG otherwise); nparam and nbin the handle's.  Per cell,
 * every product, sum and quotient rounded on its own, W the total weight:
 *   M2 == 0:  eta_p = 0 for every p, dom = 255
 *   else      var = M2 / W;  per p, s = +0.0 and over the bins with Wb > 0 in ascending order
 *               mb = S_pb / Wb;  d = mb - mean;  q = d d;  q = Wb q;  s = s + q
 *             eta_p = min((s / W) / var, 1), and exactly 0 where fewer than two bins of p have Wb > 0 (a scalar
 *             that never left one bin: nothing lies between bins, and S / W is not the mean bit for bit)
 *             dom = the lowest p that maximises eta_p, compared by a strict > in index order (255 where every
 *             eta_p is 0)
 * PS_ERR_STATE at W = 0.  Any later add, merge or reset invalidates the result. */
int ps_depend_finalize(ps_depend* h, int nparam, int nbin, const double* Wb);
/* one slot to the host (synchronises): what 0 mean, 1 variance M2 / W, 2 dom as doubles (-1 for 255), 3 M2 as
 * it is, 16 + p eta_p, 256 + 16 p + b the plane S[p][b] as it is.  PS_ERR_STATE at W = 0, and for 2 and 16 + p
 * unless finalized since the last change. */
int ps_depend_fetch(ps_depend* h, int slot, int what, double* out /* N*N */);
int ps_depend_info(ps_depend* h, double* total_weight, int64_t* members);
int ps_depend_reset(ps_depend* h);
/* measurement: HIP-event timing of the add launches, as ps_summary_prof */
int ps_depend_prof(ps_depend* h, int enable, double* total_ms, int64_t* launches);
void ps_depend_destroy(ps_depend* h);

/* ---- paired contrast of two release plans (or two projections): A - B member by member ----
 * (no reference counterpart.)  Both plans are driven by the same member, so the posterior of their
 * difference -- its variance, P(A beats B) at a cell, P(A covers more than B) -- needs the pairing and cannot
 * be rebuilt from the two plans' own maps.  The handle lives on one device and holds nslot slots of N x N
 * cells (pitch as ps_summary): mean[slot], M2[slot] (fp64) of d = a - b, and uint32 counts
 * cnt[slot][2 + 2 nthr]: plane 0 the weight of the members with d > 0, plane 1 with d < 0, plane 2 + 2k with
 * a >= t_k && b < t_k (gain_k), plane 3 + 2k with b >= t_k && a < t_k (loss_k); and with nthr > 0 per member,
 * in add order, one row uint32 [2][nthr][nslot]: the cells with a >= t_k, then those with b >= t_k, per slot
 * -- the area each plan covers, paired -- with the member's weight (the rows grow by doubling, as ps_arrival's).
 * 0 <= nthr <= 4, the thresholds finite, > 0 and strictly increasing; nslot >= 1.  The footprint,
 * (16 + 4 (2 + 2 nthr)) * nslot * pitch bytes and the first rows, is checked against the free device memory
 * first: PS_ERR_OOM before anything is allocated.  Host side: the total weight W (< 2^32) and the member
 * count.  Every mean, M2 and count cell has one writer; the rows are integer sums (ballot popcounts kept in
 * a register, summed over the block's waves in LDS, one integer atomic per block and counter): no
 * floating-point atomics, and no order of adds or merges changes a bit of a count. */
typedef struct ps_contrast ps_contrast;
int ps_contrast_create(int device, int N, int nslot, int nthr, const double* thr, ps_contrast** out);
/* One member with weight >= 1: slot e takes a = A.Y_e and b = B.Y_e of the two sources' current outputs.  Per
 * cell d = a - b (one rounded subtraction), then with W' = W + w the statements of ps_summary_add on d:
 *   d == mean: nothing stored; else mean += (d - mean) w / W',  M2 += w (d - mean_before) (d - mean)
 * and the counts above.  On the handle's stream behind both sources' last operation; their next apply waits
 * for the read.  PS_ERR_BAD_ARG (nothing enqueued): a == b, a source whose device, N or number of outputs is
 * not the handle's, weight 0 or a total weight past 2^32 - 1.  PS_ERR_STATE: a source without finished
 * fields (never applied, or a release plan mid-pass over its groups). */
int ps_contrast_add_sites(ps_contrast* h, ps_sites* a, ps_sites* b, uint32_t weight);
int ps_contrast_add_project(ps_contrast* h, ps_project* a, ps_project* b, uint32_t weight);
/* dst += src (mean and M2 as ps_summary_merge, counts added, src's rows appended after dst's), same device,
 * N, slots and thresholds; src stays as it is.  Into an empty dst it is a device copy, bit for bit. */
int ps_contrast_merge(ps_contrast* dst, ps_contrast* src);
int ps_contrast_info(ps_contrast* h, double* total_weight, int64_t* members);
/* one slot to the host (synchronises): what 0 mean, 1 variance M2 / W, 2 P(d > 0), 3 P(d < 0), 4 + 2k P(gain_k),
 * 5 + 2k P(loss_k) (count / W).  PS_ERR_STATE at W = 0. */
int ps_contrast_fetch(ps_contrast* h, int slot, int what, double* out /* N*N */);
/* the raw count plane which = what - 2 of ps_contrast_fetch */
int ps_contrast_fetch_counts(ps_contrast* h, int slot, int which, uint32_t* out /* N*N */);
/* the rows of the members first .. first + count - 1 in add order and their weights (either may be null) */
int ps_contrast_fetch_coverage(ps_contrast* h, int64_t first, int64_t count,
                               uint32_t* cells /* [count][2][nthr][nslot] */, uint32_t* weights);
int ps_contrast_reset(ps_contrast* h);
/* measurement: HIP-event timing of the add launches, as ps_summary_prof */
int ps_contrast_prof(ps_contrast* h, int enable, double* total_ms, int64_t* launches);
void ps_contrast_destroy(ps_contrast* h);

/* ---- ranking of several named release plans (or projections), member by member ----
 * (no reference counterpart.)  P plans (2..8, fixed at create) are driven by the same member.  With a_j the
 * value plan j holds at a cell (finite and >= 0 by construction of both sources), m = max_j a_j (exact) and
 * n_max the number of plans with a_j == m, the handle keeps per slot and cell
 *   best_j  += w where a_j == m and n_max == 1 (a tie counts for nobody: most of the domain is 0 for every plan),
 *   the weighted mean and M2 of the regret r_j = m - a_j (one rounded subtraction, >= 0) by the step of
 *   ps_summary_add, nothing stored where r_j equals its mean,
 * and per threshold t_k (0..4, finite, > 0, strictly increasing), with n the number of plans with a_j >= t_k,
 *   sole_kj += w where a_j >= t_k and n == 1,   any_k += w where n >= 1,   all_k += w where n == P,
 * and per member one row [P][nthr][nslot] of uint32: the cells with a_j >= t_k, kept in add order with the
 * member's weight (no rows without thresholds; the store grows by doubling).  The count planes of a slot, in
 * order: best_0 .. best_{P-1}, then per k: sole_k0 .. sole_k,P-1, any_k, all_k -- Q = P + nthr (P + 2) planes.
 * Device memory: nslot x pitch x (16 P + 4 Q) bytes, checked against the free memory before anything is
 * allocated (PS_ERR_OOM).  Every mean, M2 and count cell has one writer; the rows are integer sums (ballot
 * popcounts kept in registers, summed over the block's waves in LDS, one integer atomic per block and
 * counter): no floating-point atomics, and no order of adds or merges changes a bit of a count.
 * PS_ERR_BAD_ARG: nplan outside 2..8, nthr outside 0..4, bad thresholds. */
typedef struct ps_rank ps_rank;
int ps_rank_create(int device, int N, int nplan, int nslot, int nthr, const double* thr, ps_rank** out);
/* One member with weight >= 1: slot e takes a_j = plans[j].Y_e of the sources' current outputs.  Enqueued on
 * the handle's stream behind every source's last operation; the next apply of any source waits for the read.
 * PS_ERR_BAD_ARG (nothing enqueued): nplan outside 2..8 or not the handle's, a null or repeated source, a source
 * whose device, N or number of outputs is not the handle's, weight 0 or a total weight past 2^32 - 1.
 * PS_ERR_STATE: a source without finished fields (never applied, or a release plan mid-pass over its groups). */
int ps_rank_add_sites(ps_rank* h, ps_sites* const* plans, int nplan, uint32_t weight);
int ps_rank_add_project(ps_rank* h, ps_project* const* plans, int nplan, uint32_t weight);
/* dst += src (every mean and M2 as ps_summary_merge, counts added, src's rows appended after dst's), same
 * device, N, plans, slots and thresholds; src stays as it is.  Into an empty dst it is a device copy, bit for
 * bit. */
int ps_rank_merge(ps_rank* dst, ps_rank* src);
int ps_rank_info(ps_rank* h, double* total_weight, int64_t* members);
/* one slot of one plan to the host (synchronises): what 0 regret mean, 1 regret variance M2 / W, 2 P(best)
 * (best_j / W).  PS_ERR_BAD_ARG for a bad slot, plan or quantity; PS_ERR_STATE at W = 0. */
int ps_rank_fetch(ps_rank* h, int slot, int plan, int what, double* out /* N*N */);
/* the raw count plane `which` (0 .. Q - 1, in the order above) of a slot */
int ps_rank_fetch_counts(ps_rank* h, int slot, int which, uint32_t* out /* N*N */);
/* the rows of the members first .. first + count - 1 in add order and their weights (either may be null) */
int ps_rank_fetch_coverage(ps_rank* h, int64_t first, int64_t count,
                           uint32_t* cells /* [count][P][nthr][nslot] */, uint32_t* weights);
int ps_rank_reset(ps_rank* h);
/* measurement: HIP-event timing of the add launches, as ps_summary_prof */
int ps_rank_prof(ps_rank* h, int enable, double* total_ms, int64_t* launches);
void ps_rank_destroy(ps_rank* h);

/* ---- Monte Carlo error of the posterior maps: batch means of one sequence of members ----
 * (no reference counterpart: it calls pm.gelman_rubin on scalar parameters only.)  Every map above is a Monte
 * Carlo estimate from a correlated chain; its error needs the order of the chain at every cell and cannot be
 * rebuilt from the saved maps.  One handle is one sequence -- a chain, or half of one -- cut into batches of
 * exactly b = batch_weight rows of weight (1 .. 2^32 - 1, fixed at create).  It lives on one device and holds
 * nslot slots of N x N cells (pitch as ps_summary): fp64 bmean, bM2 (the open batch), gmean, gM2 (Welford over
 * the closed batches' means, weight 1 each), wM2 (the sum of the closed batches' own M2), and per threshold
 * uint32 bcnt (the open batch's weight with value >= t_k), uint32 s1 (the sum of the closed batches' counts)
 * and uint64 s2 (the sum of their squares).  0 <= nthr <= 4, the thresholds finite and strictly increasing.
 * The footprint, (40 + 16 nthr) * nslot * pitch bytes and one plane for the R-hat, is checked against the free
 * device memory first: PS_ERR_OOM before anything is allocated.  Every plane is zero after create and reset.
 * Host side: the closed batches B, the open batch's weight, the discarded weight and the member count; the
 * total weight added stays <= 2^32 - 1, so s2 <= n b < 2^64 with n = b B.  Every cell has one writer: no atomics
 * of either kind, and the counts are exact. */
typedef struct ps_mcerr ps_mcerr;
int ps_mcerr_create(int device, int N, int nslot, int nthr, const double* thr, uint32_t batch_weight,
                    ps_mcerr** out);
/* One member with weight >= 1, value and arguments as ps_summary_add (same value bit for bit).  The library
 * splits the weight at the batch boundaries: it fills the open batch and closes it, then whole batches of b,
 * then the rest, one launch of the add kernel per piece on the same source -- a caller that splits the weight
 * itself gets the same bits.  A piece of weight w into an open batch of weight Wo: with W' = Wo + w the
 * statements of ps_summary_add on (bmean, bM2), and bcnt_k += w where value >= t_k.  A batch that reaches b is
 * closed on the same stream, per cell: the Welford step of (gmean, gM2) with value bmean, weight 1 and B + 1
 * batches; wM2 += bM2; s1_k += bcnt_k, s2_k += bcnt_k^2; the batch planes zero again.  PS_ERR_BAD_ARG (nothing
 * enqueued): as ps_summary_add, and a total weight past 2^32 - 1. */
int ps_mcerr_add(ps_mcerr* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                 const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                 uint32_t weight);
/* the same for the current outputs of a projection or a release plan, as ps_summary_add_project /
 * ps_summary_add_sites take them */
int ps_mcerr_add_project(ps_mcerr* h, ps_project* p, uint32_t weight);
int ps_mcerr_add_sites(ps_mcerr* h, ps_sites* p, uint32_t weight);
/* discard the open batch: its planes zero, its weight onto the discarded weight */
int ps_mcerr_finish(ps_mcerr* h);
/* dst += src, pooling the closed batches: (gmean, gM2) by the expressions of ps_summary_merge with the batch
 * counts, wM2, s1 and s2 added; discarded weight and members add.  Into a dst without batches it is a device
 * copy, bit for bit.  PS_ERR_BAD_ARG: dst == src, another device, N, slot count, batch weight or thresholds;
 * PS_ERR_STATE: either handle has an open batch. */
int ps_mcerr_merge(ps_mcerr* dst, ps_mcerr* src);
/* closed batches B, b, the used weight n = b B, the open and the discarded weight, members (any may be null) */
int ps_mcerr_info(ps_mcerr* h, int64_t* batches, int64_t* batch_weight, int64_t* used_weight,
                  int64_t* open_weight, int64_t* discarded_weight, int64_t* members);
/* one raw plane of one slot to the host (synchronises): what 0 gmean, 1 gM2, 2 wM2.  PS_ERR_STATE with fewer
 * than 2 closed batches. */
int ps_mcerr_fetch(ps_mcerr* h, int slot, int what, double* out /* N*N */);
/* s1 and s2 of threshold k (either may be null); PS_ERR_STATE with fewer than 2 closed batches */
int ps_mcerr_fetch_counts(ps_mcerr* h, int slot, int k, uint32_t* s1 /* N*N */, uint64_t* s2 /* N*N */);
/* Split R-hat of one slot over 2 <= nh <= 16 sequences of the same device, N, slot count and b, each without an
 * open batch and with >= 2 closed batches (else PS_ERR_STATE); the batch counts may differ.  Per cell, the
 * sequences in argument order: mu_j = gmean_j, s2_j = (wM2_j + b gM2_j) / (n_j - 1), W = mean s2_j,
 * Bv = sum (mu_j - mean mu)^2 / (nh - 1), nbar = mean n_j, R = sqrt(((nbar - 1) / nbar W + Bv) / W), 0 where
 * W == 0.  Computed into a device plane of the first handle, one copy to the host (synchronises). */
int ps_mcerr_rhat(ps_mcerr* const* handles, int nh, int slot, double* out /* N*N */);
int ps_mcerr_reset(ps_mcerr* h);
/* measurement: HIP-event timing of the add launches (one pair per piece) and of the close launches */
int ps_mcerr_prof(ps_mcerr* h, int enable, double* add_ms, int64_t* add_launches, double* close_ms,
                  int64_t* close_launches);
void ps_mcerr_destroy(ps_mcerr* h);

/* ---- weather and parameter variance of the posterior maps: members in groups ----
 * (no reference counterpart.)  A weather ensemble evaluates every parameter vector under several wind
 * sequences; the members of one vector are a group.  Per slot and cell, fp64 planes of [slot][pitch], pitch =
 * N*N rounded up to 64 cells: imean, iM2 -- the open group, its draws with weight 1 each; omean, oM2 -- Welford
 * over the closed groups' means with weights w_g; wS = sum w_g s2_g; and the three planes finalize leaves: 8
 * planes x 8 B per cell and slot (739 MB at R = 400, 18 days; PS_ERR_OOM from a size check before anything is
 * allocated).  Host side: the open group's draws k, the closed groups G, their weight W, sum w_g / k_g and the
 * members (draws added).  Every operation is rounded on its own (no contraction), so the statements below,
 * executed one operation at a time in IEEE double, give every plane bit for bit:
 *   add (k' = k + 1):  d = v - imean;  if d != 0:  imean' = imean + d / k';  iM2 = iM2 + d * (v - imean')
 *   close(w), k >= 2:  s2 = iM2 / (k - 1);  wS = wS + w * s2;  Wn = W + w;  d = imean - omean
 *                      if d != 0:  omean' = omean + (d * w) / Wn;  oM2 = oM2 + (w * d) * (imean - omean')
 *                      imean = iM2 = +0.0
 *   merge (no open group on either side): d = omean_b - omean_a;  omean_a += d * (Wb / W);
 *                      oM2_a = (oM2_a + oM2_b) + (d * d) * ((Wa * Wb) / W);  wS_a += wS_b, W = Wa + Wb (the
 *                      expressions of ps_depend_merge); into a destination without groups a device copy
 *   finalize (G >= 2, no open group), kinv = (sum w_g / k_g) / W from the host:
 *                      vw = wS / W;  vm = oM2 / W;  vp = vm - vw * kinv;  if not (vp > 0): vp = +0.0
 *                      tot = vp + vw;  share = tot > 0 ? vw / tot : +0.0
 * vw is the variance over the wind at fixed parameters; vp the variance of the parameters' effect, the one-way
 * random-effects estimate (the between-group variance less the share of the within-group variance that the
 * group means of k_g draws carry) with the package's / W convention, clipped at 0.  One thread owns a pair of
 * cells (16-byte accesses; the tail cell of the odd N*N has its own thread), one launch covers all pairs: no
 * atomics, no LDS, and a pair where nothing changes is not stored. */
typedef struct ps_nested ps_nested;
int ps_nested_create(int device, int N, int nslot, ps_nested** out);
/* One draw of the open group, value and arguments as ps_summary_add (same value bit for bit), weight 1.
 * Enqueued on the solver's stream; no host synchronisation. */
int ps_nested_add(ps_nested* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                  const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* One draw whose values are the current outputs of a projection / a release plan (slot e takes Y_e), on the
 * handle's stream behind the source's last operation.  PS_ERR_BAD_ARG: outputs, device or domain not the
 * handle's; PS_ERR_STATE: a source without finished fields. */
int ps_nested_add_project(ps_nested* h, ps_project* p);
int ps_nested_add_sites(ps_nested* h, ps_sites* p);
/* The open group becomes a closed group of weight >= 1.  PS_ERR_STATE: fewer than 2 draws in it. */
int ps_nested_close(ps_nested* h, uint32_t weight);
/* dst += src.  PS_ERR_BAD_ARG: null, the same handle, or handles that differ in device, domain or slots;
 * PS_ERR_STATE: an open group on either side. */
int ps_nested_merge(ps_nested* dst, ps_nested* src);
/* vw, vp and share of the present groups.  PS_ERR_STATE: an open group, or fewer than 2 closed groups. */
int ps_nested_finalize(ps_nested* h);
/* total_weight: W; members: draws added; groups: G; open_draws: k; weight_per_draws: sum w_g / k_g */
int ps_nested_info(ps_nested* h, double* total_weight, int64_t* members, int64_t* groups, int64_t* open_draws,
                   double* weight_per_draws);
/* One plane of one slot (synchronises): 0 imean, 1 iM2, 2 omean, 3 oM2, 4 wS at any time; 5 vw, 6 vp, 7 share
 * after ps_nested_finalize -- PS_ERR_STATE once an add, close or merge has followed it. */
int ps_nested_fetch(ps_nested* h, int slot, int what, double* out /* N*N */);
int ps_nested_reset(ps_nested* h);
/* measurement: HIP-event timing of the add launches and of the close launches */
int ps_nested_prof(ps_nested* h, int enable, double* add_ms, int64_t* add_launches, double* close_ms,
                   int64_t* close_launches);
void ps_nested_destroy(ps_nested* h);

/* ---- posterior peak maps: how high each cell gets, on which day, and for how many days it stays above ----
 * (no reference counterpart).  Per member reductions along time: max_s v_s is not linear, so neither E[max] nor
 * the distribution of the peak day or of the days above a density can be rebuilt from the per-day maps.  A handle
 * lives on one device and holds nslot day slots (1..32, ascending) of N x N cells and 0..4 strictly increasing
 * thresholds t_0 < ... < t_{K-1}, each finite and > 0.  For one member, v_s(c) is the value ps_summary_add adds
 * for slot s (same arguments, same value bit for bit), and
 *   peak value   m(c) = max(+0.0, max_s v_s(c)): from m = +0.0, updated in slot order by the strict test v > m
 *   peak slot    p(c) = the first slot that attains m; "none" where m == 0 (not stored)
 *   duration     dur_k(c) = #{s : v_s(c) >= t_k}, 0..nslot: the listed slots, days only if they are consecutive
 * State (pitch as ps_summary): Y[pitch] fp64, the peak field of the last member added (every add rewrites it,
 * zeros included); pk[slot][pitch] uint32, the weight of the members whose peak falls on that slot;
 * du[k][n - 1][pitch] uint32, n = 1..nslot, the weight of the members with dur_k = n (n = 0 is W - the rest, not
 * stored).  The whole size, (1 + K) * nslot * pitch * 4 B plus two fp64 planes, is checked against the free
 * device memory first: PS_ERR_OOM before anything is allocated.  Host side: W (< 2^32) and the member count.
 * Counts are integers and every cell has one writer, no atomics: neither the order of adds, nor that of merges,
 * nor the launch configuration changes a bit.  Every operation records an event the next one waits on, whichever
 * stream it runs on (the solver's for add, the handle's own otherwise). */
typedef struct ps_peak ps_peak;
int ps_peak_create(int device, int N, int nslot, int nthr, const double* thr, ps_peak** out);
/* One member with weight >= 1 (arguments and refusals as ps_arrival_add): one launch on the solver's stream walks
 * every slot of every cell pair -- no early exit, the maximum needs them all -- no host synchronisation.  Every
 * descriptor is resolved first, so an add with a bad slot enqueues nothing. */
int ps_peak_add(ps_peak* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                uint32_t weight);
/* The same for the current outputs of a projection or a release plan, as ps_arrival_add_project /
 * ps_arrival_add_sites: slot e takes Y_e (nslot must equal nout), on the handle's stream. */
int ps_peak_add_project(ps_peak* a, ps_project* p, uint32_t weight);
int ps_peak_add_sites(ps_peak* a, ps_sites* p, uint32_t weight);
/* dst += src (an integer plane add), same device, N, slots and thresholds; src unchanged, dst's Y untouched */
int ps_peak_merge(ps_peak* dst, ps_peak* src);
int ps_peak_info(ps_peak* a, double* total_weight, int64_t* members);
/* zero counts, W and members; the peak field is PS_ERR_STATE again until the next add */
int ps_peak_reset(ps_peak* a);
/* the last member's peak field (synchronises).  PS_ERR_STATE before the first add. */
int ps_peak_fetch_field(ps_peak* a, double* out /* N*N */);
/* count plane pk[slot] (synchronises) */
int ps_peak_fetch_day_counts(ps_peak* a, int slot, uint32_t* out /* N*N */);
/* count plane of threshold k and duration n in 0..nslot; n == 0: W - the rest (synchronises) */
int ps_peak_fetch_duration_counts(ps_peak* a, int k, int n, uint32_t* out /* N*N */);
/* P(peak by slot) = (double)C[slot] / (double)W per cell, C[s] = sum over s' <= s of pk (synchronises; cells that
 * never hold anything stay below 1).  PS_ERR_STATE at W = 0, as every map below. */
int ps_peak_day_prob(ps_peak* a, int slot, double* out /* N*N */);
/* the smallest slot s with (double)C[s] >= p * (double)W per cell, -1 where even the last slot falls short;
 * p in (0, 1] (synchronises) */
int ps_peak_day_quantile(ps_peak* a, double p, int32_t* out /* N*N */);
/* P(dur_k >= n) = (double)(sum over n' >= n of du[k][n']) / (double)W, n in 1..nslot (synchronises) */
int ps_peak_duration_prob(ps_peak* a, int k, int n, double* out /* N*N */);
/* the smallest n in 0..nslot whose cumulative count, the implied n = 0 plane included, reaches p W by the same
 * rule; p in (0, 1] (synchronises) */
int ps_peak_duration_quantile(ps_peak* a, int k, double p, int32_t* out /* N*N */);
/* (double)(sum over n of n * du[k][n]) / (double)W, the sum exact in 64-bit integers (synchronises) */
int ps_peak_duration_mean(ps_peak* a, int k, double* out /* N*N */);
/* measurement: HIP-event timing of the add launches and of the map launches (prob, quantile, mean, n = 0 counts).
 * enable 1 on, 0 off, < 0 unchanged; the totals so far go to the non-NULL outputs (synchronises).  Finished
 * event pairs are folded into running totals, on every read and once 256 are pending, so a profiled handle
 * holds a bounded number of events however long it lives. */
int ps_peak_prof(ps_peak* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps);
void ps_peak_destroy(ps_peak* a);
/* One member with weight >= 1 whose value is the peak field of the handle's last add, as the add_project entry
 * points take a projection's outputs: the accumulator must have one slot; on the accumulator's stream behind the
 * peak add, and the next peak add waits for it.  PS_ERR_STATE before the first add. */
int ps_summary_add_peak(ps_summary* a, ps_peak* p, uint32_t weight);
int ps_hist_add_peak(ps_hist* h, ps_peak* p, uint32_t weight);

/* ---- joint excursion sets and contour credible bands: where all cells exceed t at the same time ----
 * (no reference counterpart; Bolin & Lindgren 2015, on the parametric family of the marginal level sets.)  Every
 * other map is marginal in space; the probability that all cells of a region hold >= t jointly needs each
 * member's exceedance pattern, which the per-day maps have lost.  A handle lives on one device and holds nslot
 * day slots (1..32, ascending) of N x N cells and 1..4 strictly increasing thresholds, each finite and > 0.
 * For one plane (k, slot), members m in add order with weights w_m, W their sum, v the value ps_summary_add adds:
 *   mask     B_m(c) = [v_slot^m(c) >= t_k]
 *   count    C(c) = sum_m w_m B_m(c)                               (W x the summary's exceedance)
 *   bounds   hi_m = max{C(c) : B_m(c) = 0}, 0 if there is no such cell with C > 0
 *            lo_m = min{C(c) : B_m(c) = 1}, 0xffffffff if the mask is empty
 *   above    A+(c) = sum_m w_m [hi_m < C(c)] where C(c) > 0, else 0
 *   below    A-(c) = sum_m w_m [lo_m > C(c)]
 *   contour  u = min(C, W - C); Ac(c) = sum_m w_m [hi_m < W - u and lo_m > u] where 2u < W, else 0
 * and every map is (double)A / (double)W.  Member m exceeds on the whole level set {C >= n} iff hi_m < n and is
 * below on the whole of {C <= n} iff lo_m > n, so {A+ / W >= level} is the largest level set of C on which all
 * cells exceed t jointly with probability >= level, {A- / W >= level} its mirror image, and {Ac / W < level}
 * the credible band of the t-contour.  State (pitch as ps_summary, nword = pitch / 64): cnt[k][slot][pitch]
 * uint32; mask[member][k][slot][nword] uint64, bit l of word j the cell 64 j + l (pad bits 0), which grows by
 * doubling; the weights on the host.  The counts and one fp64 plane are checked against the free device memory
 * at create, every growth of the masks when it happens: PS_ERR_OOM before anything is allocated.  W < 2^32 - 1
 * (the value 0xffffffff is lo's "no cell").  Counts and masks have one writer per word, the bounds are integer
 * maxima and minima (integer atomics): neither the order of adds, nor that of merges, nor the launch
 * configuration changes a bit; only the order of the members in the fetches follows the adds.  Every operation
 * records an event the next one waits on, whichever stream it runs on (the solver's for add, the handle's own
 * otherwise). */
#define PS_EXCUR_ABOVE 0
#define PS_EXCUR_BELOW 1
#define PS_EXCUR_CONTOUR 2
typedef struct ps_excur ps_excur;
int ps_excur_create(int device, int N, int nslot, int nthr, const double* thr, ps_excur** out);
/* room for `members` members' masks now (a growth synchronises; never shrinks) */
int ps_excur_reserve(ps_excur* a, int64_t members);
/* One member with weight >= 1 (arguments and refusals as ps_arrival_add, and a total weight past 2^32 - 2): one
 * launch on the solver's stream, one thread per cell, every slot of every cell and every mask word of the member
 * written, zeros included; no host synchronisation unless the masks have to grow.  Every descriptor is resolved
 * first, so an add with a bad slot enqueues nothing. */
int ps_excur_add(ps_excur* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                 const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                 uint32_t weight);
/* The same for the current outputs of a projection, a release plan or the peak field of a ps_peak, as
 * ps_arrival_add_project / ps_arrival_add_sites / ps_summary_add_peak: slot e takes Y_e (nslot must equal nout),
 * on the handle's stream. */
int ps_excur_add_project(ps_excur* a, ps_project* p, uint32_t weight);
int ps_excur_add_sites(ps_excur* a, ps_sites* p, uint32_t weight);
int ps_excur_add_peak(ps_excur* a, ps_peak* p, uint32_t weight);
/* dst += src: the counts by an integer plane add, src's members and weights appended after dst's (a device copy);
 * same device, N, slots and thresholds; src unchanged */
int ps_excur_merge(ps_excur* dst, ps_excur* src);
/* any pointer may be NULL; capacity: the members the masks hold room for; bytes: the device memory held now */
int ps_excur_info(ps_excur* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes);
/* zero counts, W and members; the masks keep their room */
int ps_excur_reset(ps_excur* a);
/* hi and lo of every (member, k, slot) from the counts as they are now and the stored masks, kept on the host
 * (synchronises).  The maps and ps_excur_fetch_bounds call it themselves; it does nothing while its result is
 * current, and any add, merge or reset makes it stale.  PS_ERR_STATE before the first add. */
int ps_excur_finalize(ps_excur* a);
/* one map of plane (k, slot), what = PS_EXCUR_ABOVE / _BELOW / _CONTOUR (synchronises): the host sorts the
 * members' bounds into a step table of breakpoints and exact integer cumulative weights, one thread per cell
 * searches it with C (or u).  PS_ERR_STATE before the first add. */
int ps_excur_map(ps_excur* a, int k, int slot, int what, double* out /* N*N */);
int ps_excur_fetch_counts(ps_excur* a, int k, int slot, uint32_t* out /* N*N */);
/* the mask words of one member, the pad bits included */
int ps_excur_fetch_mask(ps_excur* a, int64_t member, int k, int slot, uint64_t* out /* pitch / 64 */);
/* the bounds of plane (k, slot) and the weights, per member in add order (any pointer may be NULL) */
int ps_excur_fetch_bounds(ps_excur* a, int k, int slot, uint32_t* hi, uint32_t* lo, uint32_t* weights /* members */);
/* measurement: HIP-event timing of the add launches [0], the finalize launches [1] and the map launches [2];
 * enable 1 on, 0 off, < 0 unchanged; ms[3] / launches[3] (either may be NULL) receive the totals so far
 * (synchronises).  Finished event pairs are folded into running totals as in ps_peak_prof. */
int ps_excur_prof(ps_excur* a, int enable, double* ms /* 3 */, int64_t* launches /* 3 */);
void ps_excur_destroy(ps_excur* a);

/* ---- reweighted posterior summaries: the maps under new observations, without a new chain ----
 * (no reference counterpart.)  Every other accumulator weights a member by its run length, an integer: the maps
 * are conditional on the data the chain was fitted to.  Importance reweighting gives member m the real weight
 * n_m L_m, L_m the likelihood of new observations under the member's own fields -- which the saved maps have
 * lost.  A handle lives on one device and holds J scenarios (1..4), nslot slots (1..32) of N x N cells and K
 * thresholds (0..4, each finite and > 0, strictly increasing).  Per scenario j on the device, all fp64 (pitch as
 * ps_summary):
 *   mean[j][slot][pitch], m2[j][slot][pitch], S[j][slot][k][pitch]   (S_k: the weight of the members with v >= t_k)
 * and on the host W_j (a double, 0 while empty), members_j and skipped_j.  The whole block,
 * J * (2 + K) * 8 B * nslot * pitch, is checked against the free device memory first: PS_ERR_OOM before anything
 * is allocated.  At R = 400 (N = 801, pitch 641 664), 18 days and K = 2 one scenario takes
 * 641 664 x 18 x 32 B = 370 MB.  The likelihoods may span hundreds of orders of magnitude: the caller keeps a
 * log-scale reference per scenario and passes, per member, a rescale r in [0, 1] of what is held so far and a
 * weight omega >= 0 on the new scale, so no weight ever exceeds the run length.  One thread owns a pair of
 * cells: no atomics, the same calls in the same order give the same bits.  Every operation records an event
 * that the next one waits on, on whatever stream it runs (the solver's for add, the handle's own otherwise). */
typedef struct ps_wsum ps_wsum;
int ps_wsum_create(int device, int N, int nscen, int nslot, int nthr, const double* thr, ps_wsum** out);
/* One member from the records of solver s: the slot descriptors and the value v of a cell are those of
 * ps_summary_add (same arguments, same value bit for bit).  rescale[nscen] (r, in [0, 1]) and omega[nscen]
 * (>= 0, finite); nscen the handle's.  omega_j == 0: the member leaves scenario j untouched and skipped_j grows
 * by one.  For a scenario with omega > 0, every step a statement of its own (one rounding each, but for the
 * two statements of ps_summary_add, which contract as they do there):
 *   host:      W = W * r;  W = W + omega;
 *   per cell:  q = q * r;  S_k = S_k * r (every k);  d = v - m;
 *              d != 0:  m += d omega / W,  q += omega d (v - m)        (the statements of ps_summary_add)
 *              S_k = S_k + omega   (every k with v >= t_k)
 * so a host loop with one rounded operation per statement reproduces mean and every S_k bit for bit, and with
 * r = 1 and integer omega the handle holds the bits of a ps_summary fed alongside.  A value is stored only
 * where its bits changed, and with r == 1 a pair of cells with v == m below t_0 reads its means alone.  One launch per member on the solver's stream, no host synchronisation; the thread
 * reads the record once and walks the scenarios.  PS_ERR_BAD_ARG (every descriptor and argument is checked
 * before anything is enqueued; a refused add changes nothing): a wrong nscen or nslot, r outside [0, 1], omega
 * NaN, negative or infinite, a solver of another device or domain. */
int ps_wsum_add(ps_wsum* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                int nscen, const double* rescale, const double* omega);
/* The same member whose values are the current outputs of a projection, a release plan or the peak field of a
 * ps_peak, as ps_summary_add_project / _add_sites / _add_peak take them: slot e takes Y_e, on the handle's stream
 * behind the source's last operation; its next apply waits for the read. */
int ps_wsum_add_project(ps_wsum* h, ps_project* p, int nscen, const double* rescale, const double* omega);
int ps_wsum_add_sites(ps_wsum* h, ps_sites* p, int nscen, const double* rescale, const double* omega);
int ps_wsum_add_peak(ps_wsum* h, ps_peak* p, int nscen, const double* rescale, const double* omega);
/* dst += src per scenario, same device, N, scenarios, slots and thresholds; src stays as it is.  ra[j], rb[j] in
 * [0, 1] bring both sides to a common scale (the caller's): Wa' = Wa ra, Wb' = Wb rb, W = Wa' + Wb',
 *   d = mean_b - mean_a;  mean = mean_a + d (Wb' / W);  m2 = m2a ra + m2b rb + d^2 (Wa' Wb' / W);  S = Sa ra + Sb rb.
 * A scenario empty in src adds its skipped count alone; into a scenario empty in dst it is a device copy, bit
 * for bit, W included (ra, rb unused). */
int ps_wsum_merge(ps_wsum* dst, ps_wsum* src, const double* ra, const double* rb);
/* per scenario (any pointer may be NULL): W, members (adds with omega > 0) and skipped (adds with omega == 0) */
int ps_wsum_info(ps_wsum* h, double* total_weight /* nscen */, int64_t* members, int64_t* skipped);
/* one slot of one scenario to the host (synchronises): what 0 mean, 1 variance m2 / W, 2 + k min(S_k / W, 1.0).
 * PS_ERR_STATE while the scenario has W = 0. */
int ps_wsum_fetch(ps_wsum* h, int scen, int slot, int what, double* out /* N*N */);
int ps_wsum_reset(ps_wsum* h);
/* measurement: HIP-event timing of the add launches, as ps_summary_prof */
int ps_wsum_prof(ps_wsum* h, int enable, double* total_ms, int64_t* launches);
void ps_wsum_destroy(ps_wsum* h);

/* ---- reweighted posterior histograms: quantiles and credible bands under new observations ----
 * (no reference counterpart.)  ps_hist's per-cell histograms with the real weights of ps_wsum: J scenarios (1..4),
 * nslot slots (1..32) of N x N cells and the edge table of a ps_hist: 2 <= nedge = B + 1 <= 1024 edges, finite,
 * > 0, strictly increasing; bin b = searchsorted(edges, v, side='right'), bin 0 not stored.  Per scenario j fp64
 * planes H[j][slot][b = 1 .. B+1][pitch] on the scale exp(ref_j) the caller keeps, and per slot and cell one
 * range word of the lowest and highest touched bin as ps_hist's, shared by the scenarios (a superset is harmless:
 * untouched planes hold +0.0).  Host side per scenario W_j (a double, 0 while empty), members_j and skipped_j.
 * The full size, J * nslot * nedge * pitch * 8 B + nslot * pitch * 4 B plus scratch, is checked against the free
 * device memory first: PS_ERR_OOM before anything is allocated.  One thread owns a pair of cells: no atomics, the
 * same calls in the same order give the same bits; these are floating-point sums, so another order of adds or
 * merges moves a plane within the rounding of its sums.  Every operation records an event that the next one waits
 * on, on whatever stream it runs (the solver's for add, the handle's own otherwise). */
typedef struct ps_whist ps_whist;
int ps_whist_create(int device, int N, int nscen, int nslot, int nedge, const double* edges, ps_whist** out);
/* One member from the records of solver s (slot descriptors and the value v of a cell as ps_summary_add; rescale,
 * omega and their refusals as ps_wsum_add).  omega_j == 0: the member leaves scenario j untouched and skipped_j
 * grows by one.  For a scenario with omega > 0, every step a statement of its own (one rounding each):
 *   host:      W = W * r;  W = W + omega;
 *   per cell:  H_b = H_b * r on every plane (r != 1 only: a launch of its own over each cell's touched planes);
 *              H_b = H_b + omega for the cell's bin b >= 1
 * so a host loop with one rounded operation per statement reproduces every plane bit for bit, and with r = 1 and
 * integer omega the planes hold the counts of a ps_hist fed alongside.  The add is one launch on the solver's
 * stream that reads the record once for all scenarios; no host synchronisation.  An add refused for its arguments
 * (PS_ERR_BAD_ARG, every one checked before anything is enqueued) changes nothing; a HIP error of a launch or of a
 * profiling event after the rescale was enqueued (PS_ERR_HIP) leaves the planes rescaled and W, the members and
 * the caller's reference as they were: the handle is then to be reset. */
int ps_whist_add(ps_whist* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                 const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                 int nscen, const double* rescale, const double* omega);
/* The same member whose values are the current outputs of a projection or a release plan, as ps_hist_add_project /
 * ps_hist_add_sites take them: slot e takes Y_e, on the handle's stream behind the source's last operation; its
 * next apply waits for the read. */
int ps_whist_add_project(ps_whist* h, ps_project* p, int nscen, const double* rescale, const double* omega);
int ps_whist_add_sites(ps_whist* h, ps_sites* p, int nscen, const double* rescale, const double* omega);
/* dst += src per scenario, same device, N, scenarios, slots and edges; src stays as it is.  ra[j], rb[j] in [0, 1]
 * bring both sides to a common scale (the caller's): x = Ha ra; y = Hb rb; H = x + y (three statements), W
 * likewise; the range words take the per-half maximum.  A scenario empty in src adds its skipped count alone; into
 * a scenario empty in dst it is a device copy, bit for bit, W included. */
int ps_whist_merge(ps_whist* dst, ps_whist* src, const double* ra, const double* rb);
/* per scenario (any pointer may be NULL): W, members (adds with omega > 0) and skipped (adds with omega == 0) */
int ps_whist_info(ps_whist* h, double* total_weight /* nscen */, int64_t* members, int64_t* skipped);
/* One slot's quantile at p in (0, 1] under one scenario (synchronises; any output may be NULL).  From the cell's
 * highest touched bin down T_b = T_{b+1} + H_b (one rounded add per plane, T above the top 0) and
 * C_b = W - T_{b+1}; b* = the smallest b with C_b >= p W (bin, int32).  lower / upper: the bracket of b* as
 * ps_hist_quantile's.  value: e_{b*-1} (e_{b*} / e_{b*-1})^f, f = (p W - C_{b*-1}) / H_{b*} clamped to [0, 1], for
 * 1 <= b* <= B, 0 at b* = 0, e_B at b* = B + 1.  With integer weights every step is exact and the outputs are
 * those of ps_hist_quantile bit for bit.  PS_ERR_STATE while the scenario has W = 0. */
int ps_whist_quantile(ps_whist* h, int scen, int slot, double p, double* value, double* lower, double* upper,
                      int32_t* bin);
/* min(T_{k+1} / W, 1.0) per cell: P(v >= e_k) under the scenario, at any edge k (synchronises).  PS_ERR_STATE while
 * the scenario has W = 0. */
int ps_whist_exceed(ps_whist* h, int scen, int slot, int k, double* out /* N*N */);
/* the raw plane of bin b (1 .. B + 1) of one scenario and slot, on the scale exp(ref) (synchronises) */
int ps_whist_fetch(ps_whist* h, int scen, int slot, int b, double* out /* N*N */);
int ps_whist_reset(ps_whist* h);
/* measurement: HIP-event timing of the add launches, the quantile and exceedance launches and the rescale
 * launches.  enable 1 on, 0 off, < 0 unchanged; the totals so far go to the non-NULL outputs (synchronises). */
int ps_whist_prof(ps_whist* h, int enable, double* add_ms, int64_t* adds, double* q_ms, int64_t* q_launches,
                  double* rescale_ms, int64_t* rescales);
void ps_whist_destroy(ps_whist* h);

/* ---- reweighted posterior arrival maps: when do they reach each cell under new observations ----
 * (no reference counterpart.)  ps_arrival's arrival counts with the real weights of ps_wsum: J scenarios (1..4),
 * nslot slots (1..32) and 1..4 thresholds as ps_arrival's; a_k(c) = min{s : v_s(c) >= t_k} exactly as there.  Per
 * scenario j fp64 planes A[j][k][s][pitch]: the weight of the members with a_k(c) = s on the scale exp(ref_j);
 * "never" is W - the rest, not stored.  Host side per scenario W_j, members_j, skipped_j.  The whole block,
 * J * K * nslot * pitch * 8 B plus scratch, is checked against the free device memory first (PS_ERR_OOM).  The
 * members' reached-cell rows stay with ps_arrival.  One writer per cell, no atomics; floating-point sums as
 * ps_whist's.  Stream ordering as ps_whist. */
typedef struct ps_warr ps_warr;
int ps_warr_create(int device, int N, int nscen, int nslot, int nthr, const double* thr, ps_warr** out);
/* One member (arguments and refusals as ps_whist_add): where r != 1, A = A * r over the scenario's planes in a
 * launch of its own; then one launch walks the slots of every cell pair as ps_arrival_add does, the records read
 * once for all scenarios, and A[j][k][a_k] = A + omega_j where a_k < nslot.  Host: W = W * r; W = W + omega.  After a
 * HIP error behind an enqueued rescale the handle is to be reset, as ps_whist_add states. */
int ps_warr_add(ps_warr* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                int nscen, const double* rescale, const double* omega);
/* The same for the current outputs of a projection or a release plan, as ps_arrival_add_project / _add_sites */
int ps_warr_add_project(ps_warr* h, ps_project* p, int nscen, const double* rescale, const double* omega);
int ps_warr_add_sites(ps_warr* h, ps_sites* p, int nscen, const double* rescale, const double* omega);
/* dst += src per scenario as ps_whist_merge: x = Aa ra; y = Ab rb; A = x + y; a device copy into an empty one */
int ps_warr_merge(ps_warr* dst, ps_warr* src, const double* ra, const double* rb);
int ps_warr_info(ps_warr* h, double* total_weight /* nscen */, int64_t* members, int64_t* skipped);
/* min(C_slot / W, 1.0) per cell, C_s = C_{s-1} + A_s ascending, one rounded add each (synchronises).  PS_ERR_STATE
 * while the scenario has W = 0. */
int ps_warr_prob(ps_warr* h, int scen, int k, int slot, double* out /* N*N */);
/* the smallest slot s with C_s >= p W per cell, -1 where even the last slot falls short; p in (0, 1]
 * (synchronises).  PS_ERR_STATE while the scenario has W = 0. */
int ps_warr_quantile(ps_warr* h, int scen, int k, double p, int32_t* out /* N*N */);
/* the raw plane of threshold k and slot 0 .. nslot - 1 of one scenario, on the scale exp(ref) (synchronises) */
int ps_warr_fetch(ps_warr* h, int scen, int k, int slot, double* out /* N*N */);
int ps_warr_reset(ps_warr* h);
/* measurement: HIP-event timing of the add, map and rescale launches, as ps_whist_prof */
int ps_warr_prof(ps_warr* h, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps,
                 double* rescale_ms, int64_t* rescales);
void ps_warr_destroy(ps_warr* h);

/* ---- catch-probability fields: what a trap at each cell would find in one member's field ----
 * (no reference counterpart; the Poisson model is that of the package's own likelihood, mcmc.loglik_parts.)
 * A handle lives on one device and holds nout outputs (1..32) over nin inputs (1..32): output e is
 * (input[e], rate[e], count[e]) with 0 <= input[e] < nin, rate finite and > 0 and count a whole number in 1..16
 * (PS_ERR_BAD_ARG otherwise), and nout fp64 fields Y[e][pitch] (pitch as ps_summary), whose size, nout * pitch
 * * 8 B, is checked against the free device memory first: PS_ERR_OOM before anything is allocated.  With v the
 * value of input[e] at a cell, an apply overwrites every cell of every output, zeros included, with
 *   Y_e(c) = P(Poisson(mu) >= n),   mu = rate[e] * v   (one rounded product),   n = count[e]
 * evaluated by these statements, one IEEE double rounding each (never fused), exp and expm1 the device library's:
 *   not (mu > 0):   Y = +0.0               (so Y is exactly +0.0 where v == 0; every other value lies in [0, 1])
 *   mu >= 800:      Y = 1.0                (exp(-mu) is 0 from 746 on)
 *   n == 1:         x = expm1(-mu);  Y = -x
 *   mu < n:         t = 1;  for i = 1..n:  t = t * mu;  t = t / i               (mu^n / n! as a running product)
 *                   s = 1;  u = 1;  for j = 1..56:  r = mu / (n + j);  u = u * r;  s = s + u
 *                   t = t * s;  e = exp(-mu);  Y = t * e;  Y > 1: Y = 1
 *   mu >= n:        u = 1;  q = 1;  for i = 1..n-1:  u = u * mu;  u = u / i;  q = q + u
 *                   e = exp(-mu);  p = e * q;  Y = 1 - p;  Y < 0: Y = 0        (Y >= about 0.45: nothing cancels)
 * The device leaves the series at the first term that does not change s; every later term is smaller, so the
 * 56 terms give the same bits, and the stop depends on the cell's own (mu, n) alone: neither grid nor block
 * shape changes a bit.  One thread owns a pair of cells (the tail cell of an odd N * N alone); the outputs are
 * grouped by input, so a record is read once however many outputs use it; a pair whose values are both zero
 * writes zeros without touching the exponential path.  No atomics, one writer per cell.  Every operation
 * records an event the next one waits on, whichever stream it runs on (the solver's for ps_catch_apply, the
 * handle's own for the other applies, fetch and gather, the accumulator's for the _add_catch entry points). */
typedef struct ps_catch ps_catch;
int ps_catch_create(int device, int N, int nin, int nout, const int32_t* input /* nout */,
                    const double* rate /* nout */, const int32_t* count /* nout */, ps_catch** out);
/* The inputs are records of solver s (same device, same N; arguments as ps_project_apply, nin must equal the
 * handle's; v is the value ps_summary_add adds, bit for bit): one launch on the solver's stream, no host
 * synchronisation, nothing copied or allocated. */
int ps_catch_apply(ps_catch* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                   const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* The inputs are the current outputs of a projection or a release plan: input i is the source's output i, so
 * nin must equal its nout, and device and N must agree (PS_ERR_BAD_ARG, nothing enqueued); PS_ERR_STATE before
 * the source's first apply.  One launch on the handle's stream behind the source's last operation; the source's
 * next apply waits for the read. */
int ps_catch_apply_project(ps_catch* c, ps_project* p);
int ps_catch_apply_sites(ps_catch* c, ps_sites* p);
/* one output field to the host (synchronises).  PS_ERR_STATE before the first apply. */
int ps_catch_fetch(ps_catch* c, int e, double* out /* N*N */);
/* the outputs at n listed cells: out[e * n + k] = Y_e(rows[k], cols[k]) (synchronises).  PS_ERR_BAD_ARG for
 * a cell outside the domain, PS_ERR_STATE before the first apply. */
int ps_catch_gather(ps_catch* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out /* nout x n */);
/* any pointer may be NULL */
int ps_catch_info(ps_catch* c, int* N, int* nin, int* nout, int64_t* applies);
/* measurement: HIP-event timing of the apply launches.  enable 1 on, 0 off, < 0 unchanged; total_ms /
 * launches (either may be NULL) receive the timed launches so far (synchronises).  Finished event pairs are
 * folded into running totals as in ps_peak_prof. */
int ps_catch_prof(ps_catch* c, int enable, double* total_ms, int64_t* launches);
void ps_catch_destroy(ps_catch* c);
/* One member whose values are the handle's current outputs, as ps_summary_add_project / ps_mcerr_add_project /
 * ps_wsum_add_project take a projection's: slot e takes Y_e, through the accumulator's own add kernel, on the
 * accumulator's stream behind the handle's last operation; the next apply waits for the read.  The
 * accumulator's slot count must equal nout, device and N must agree (PS_ERR_BAD_ARG, nothing enqueued);
 * PS_ERR_STATE before the first apply. */
int ps_summary_add_catch(ps_summary* a, ps_catch* c, uint32_t weight);
int ps_mcerr_add_catch(ps_mcerr* h, ps_catch* c, uint32_t weight);
int ps_wsum_add_catch(ps_wsum* h, ps_catch* c, int nscen, const double* rescale, const double* omega);

/* ---- trap information fields: how much a catch at each cell would teach ----
 * (no reference counterpart; the Poisson model is that of the package's own likelihood, mcmc.loglik_parts.)
 * The mutual information between a trap's count and the identity of the ensemble member: where it is large a
 * reading separates the members, where it is 0 -- on the release point as outside every plume -- it separates
 * none.  It equals the expected Kullback-Leibler divergence from today's posterior to the reweighted posterior
 * (ps_wsum) after the reading.  A handle lives on one device and holds ntrap traps over nin inputs (1..32): trap
 * e is (input[e], rate[e], ymax[e]) with 0 <= input[e] < nin, rate finite and > 0 and ymax a whole number in
 * 0..15 (PS_ERR_BAD_ARG otherwise).  The trap's count is observed as the classes 0, 1, .., ymax and
 * ">= ymax + 1"; ymax = 0 is the found / none trap.  Trap e owns ymax[e] + 3 consecutive fp64 planes [pitch]
 * (pitch as ps_summary), in the caller's order; at most 32 planes in all, the slots of one accumulator
 * (PS_ERR_BAD_ARG beyond).  The planes and three result maps per trap, (nplane + 3 ntrap) * pitch * 8 B, are
 * checked against the free device memory first: PS_ERR_OOM before anything is allocated.  With v the value of
 * input[e] at a cell and mu = rate[e] * v (one rounded product), an apply overwrites every cell of every plane
 * of the trap by these statements, one IEEE double rounding each (never fused), exp, expm1 and log the device
 * library's, catch_value the statements of the ps_catch block above:
 *   not (mu > 0):  every plane +0.0
 *   mu >= 800:     d0 = 1;  p_y = 0;  tail = 1;  h = 0
 *   else:          nm = -mu;  x = expm1(nm);  d0 = -x;  e = exp(nm);  h = e * mu;  t = e
 *                  for y = 1..ymax:  t = t * mu;  t = t / y;  p_y = t;
 *                                    if t > 0:  l = log(t);  x = t * l;  h = h - x
 *                  q = catch_value(mu, ymax + 1);  tail = q
 *                  if q > 0:  l = log(q);  x = q * l;  h = h - x
 * The planes in order: d0 = 1 - P(count = 0), stored as this deficit so that every plane is exactly +0.0 where
 * v == 0; p_1 .. p_ymax; tail = P(count >= ymax + 1); h, the entropy in nats of this member's class
 * distribution.  One thread owns a pair of cells (the tail cell of an odd N * N alone); the traps are grouped by
 * input, so a record is read once however many traps use it; a pair whose values are both zero writes zeros
 * without touching the transcendental path.  No atomics, one writer per cell; neither grid nor block shape
 * changes a bit.  Every operation records an event the next one waits on, whichever stream it runs on (the
 * solver's for ps_gain_apply, the handle's own for the other applies, finish, fetch and gather, the
 * accumulator's for the _add_gain entry points). */
typedef struct ps_gain ps_gain;
int ps_gain_create(int device, int N, int nin, int ntrap, const int32_t* input /* ntrap */,
                   const double* rate /* ntrap */, const int32_t* ymax /* ntrap */, ps_gain** out);
/* The inputs are records of solver s (same device, same N; arguments as ps_project_apply, nin must equal the
 * handle's; v is the value ps_summary_add adds, bit for bit): one launch on the solver's stream, no host
 * synchronisation, nothing copied or allocated. */
int ps_gain_apply(ps_gain* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                  const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* The inputs are the current outputs of a projection or a release plan: input i is the source's output i, so
 * nin must equal its nout, and device and N must agree (PS_ERR_BAD_ARG, nothing enqueued); PS_ERR_STATE before
 * the source's first apply.  One launch on the handle's stream behind the source's last operation; the source's
 * next apply waits for the read. */
int ps_gain_apply_project(ps_gain* c, ps_project* p);
int ps_gain_apply_sites(ps_gain* c, ps_sites* p);
/* One member whose values are the handle's current planes: slot k takes plane k, through the accumulator's own
 * add kernel, as ps_summary_add_catch / ps_wsum_add_catch; the accumulator's slot count must equal the number
 * of planes.  The posterior mean of a p_y plane is then the posterior predictive probability of that class, the
 * mean of h is H(count | member). */
int ps_summary_add_gain(ps_summary* a, ps_gain* c, uint32_t weight);
int ps_wsum_add_gain(ps_wsum* h, ps_gain* c, int nscen, const double* rescale, const double* omega);
/* The three maps of every trap from the mean planes m_k of an accumulator fed by the _add_gain entry points
 * (of a ps_wsum: those of one scenario), read on the device -- slots, device and N must agree (PS_ERR_BAD_ARG,
 * nothing enqueued), PS_ERR_STATE while the accumulator is empty.  Per cell and trap, m_0 .. m_{ymax+2} the
 * trap's planes, every line a statement of its own:
 *   P0 = 1 - m_0;  HY = 0;  for P in (P0, m_1, .., m_{ymax+1}):  if P > 0:  l = log(P);  x = P * l;  HY = HY - x
 *   HYM = m_{ymax+2};  G = HY - HYM;  if not (G > 0):  G = +0.0
 * One launch on the handle's stream behind the accumulator's last operation; the accumulator's next operation
 * waits for the read.  The maps of an earlier finish are overwritten. */
int ps_gain_finish_summary(ps_gain* c, ps_summary* a);
int ps_gain_finish_wsum(ps_gain* c, ps_wsum* h, int scenario);
/* one plane of the last apply to the host, 0 <= plane < the number of planes (synchronises).  PS_ERR_STATE
 * before the first apply. */
int ps_gain_fetch(ps_gain* c, int plane, double* out /* N*N */);
/* one map of the last finish to the host: what 0 the gain G (the mutual information in nats), 1 the entropy HY
 * of the posterior predictive class distribution, 2 the conditional entropy HYM (synchronises).  PS_ERR_STATE
 * before the first finish. */
int ps_gain_fetch_result(ps_gain* c, int trap, int what, double* out /* N*N */);
/* the planes at n listed cells: out[k * n + i] = plane k at (rows[i], cols[i]) (synchronises).
 * PS_ERR_BAD_ARG for a cell outside the domain, PS_ERR_STATE before the first apply. */
int ps_gain_gather(ps_gain* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out /* nplane x n */);
/* any pointer may be NULL */
int ps_gain_info(ps_gain* c, int* N, int* nin, int* ntrap, int* nplane, int64_t* applies);
/* measurement: HIP-event timing of the apply launches, as ps_catch_prof */
int ps_gain_prof(ps_gain* c, int enable, double* total_ms, int64_t* launches);
void ps_gain_destroy(ps_gain* c);

/* ---- core-range maps: where each member holds most of its wasps ----
 * (no reference counterpart.)  Every other map cuts a member's field at an absolute density.  Here the cut is the
 * member's own: for fractions p_0 < ... < p_{J-1} (1..4, each a finite double in (0, 1)) and nslot slots (1..32) of
 * N x N cells (N * N < 2^25) the smallest region that holds the share p_j of the member's mass, the highest-density
 * region {v >= lambda_j} -- the 50 % "core" and the 95 % "range" of the utilisation distribution.  v is the value
 * ps_summary_add adds for the slot; a cell whose value is not > 0, or not finite, has mass 0 and lies in no set.  Per member and
 * slot, every line a statement of its own:
 *   vmax = max v;  not (vmax > 0): the slot is empty, lambda_j = +inf, n_j = 0, Q = 0, nothing is counted
 *   E = floor(log2 vmax), from the exponent field;  q(c) = (uint64) floor(scalbn(v(c), 36 - E)) < 2^37, exact
 *   Q = sum of q (an integer < 2^62);  need_j = the smallest integer >= p_j Q, p_j at its exact binary value
 *   lambda_j = the largest x with sum of q over {v >= x} >= need_j (a value the field holds; ties enter whole)
 *   B_j = {v >= lambda_j};  n_j = the cells of B_j;  B_0 in B_1 in ...
 * State (pitch as ps_summary): cnt[j][slot][pitch] uint32, C_j += w_m B_j; per member in add order
 * lambda[j][slot] fp64, n[j][slot] uint32, Q[slot] uint64, E[slot] int32 (grow by doubling, 12 B per member,
 * fraction and slot plus 12 B per member and slot); the weights on the host; about 1 MB of pass scratch.  No masks
 * are kept.  Every allocation is checked against the free device memory first: PS_ERR_OOM before it is made.
 * lambda is found on the device by a radix select over the 64-bit pattern of v weighted by q (positive doubles
 * order as their patterns): six passes of 10 bits over key = bits(v) - bits(2^(E-36)) < 2^60, each a histogram of
 * integer mass per digit in LDS folded to global memory and a pick kernel that extends every (slot, fraction)
 * prefix; no value comes back to the host during an add.  Integer atomics only: neither the order of adds, nor
 * that of merges, nor the launch configuration changes a bit; only the order of the members in the fetches follows
 * the adds.  Every operation records an event the next one waits on, whichever stream it runs on (the solver's
 * for add, the handle's own otherwise). */
typedef struct ps_range ps_range;
/* PS_ERR_BAD_ARG for fractions outside (0, 1), NaN, not strictly increasing, more than 4, or slots outside 1..32 */
int ps_range_create(int device, int N, int nslot, int nfrac, const double* frac, ps_range** out);
/* room for `members` members' rows now (a growth synchronises; never shrinks) */
int ps_range_reserve(ps_range* a, int64_t members);
/* One member with weight >= 1 (arguments and refusals as ps_arrival_add; a total weight past 2^32 - 1 is refused):
 * fourteen launches on the solver's stream, every slot in each; no host synchronisation unless the rows have to
 * grow.  Every descriptor is resolved first, so an add with a bad slot enqueues nothing. */
int ps_range_add(ps_range* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                 const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                 uint32_t weight);
/* The same for the current outputs of a projection or a release plan, as ps_arrival_add_project /
 * ps_arrival_add_sites: slot e takes Y_e (nslot must equal nout), on the handle's stream. */
int ps_range_add_project(ps_range* a, ps_project* p, uint32_t weight);
int ps_range_add_sites(ps_range* a, ps_sites* p, uint32_t weight);
/* dst += src: the counts by an integer plane add, src's member rows and weights appended after dst's (device
 * copies); same device, N, slots and fractions; src unchanged */
int ps_range_merge(ps_range* dst, ps_range* src);
/* any pointer may be NULL; capacity: the members the rows hold room for; bytes: the device memory held now */
int ps_range_info(ps_range* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes);
/* zero counts, W and members and drop the timings of ps_range_prof; the rows keep their room */
int ps_range_reset(ps_range* a);
/* (double)C_j[slot] / (double)W: the posterior probability that the cell lies in the member's p_j range
 * (synchronises).  PS_ERR_STATE before the first add, as the fetches below. */
int ps_range_prob(ps_range* a, int j, int slot, double* out /* N*N */);
int ps_range_fetch_counts(ps_range* a, int j, int slot, uint32_t* out /* N*N */);
/* per member in add order the level, the cells of the set and the weight (any pointer may be NULL) */
int ps_range_fetch_members(ps_range* a, int j, int slot, double* lambda, uint32_t* cells, uint32_t* weights);
/* per member in add order the integer mass Q and the exponent E of the slot (either may be NULL) */
int ps_range_fetch_mass(ps_range* a, int slot, uint64_t* Q, int32_t* E /* members */);
/* measurement: HIP-event timing of the adds and the map launches, as ps_arrival_prof; the totals count from
 * the last ps_range_reset */
int ps_range_prof(ps_range* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps);
void ps_range_destroy(ps_range* a);

/* ---- patch maps: is the reached area one front or separate foci? ----
 * (no reference counterpart.)  Every other map has lost the pairing of cells within a member; connectivity is a
 * joint statement in space about one member's field.  Inputs: thresholds t_0 < ... < t_{K-1} (K in 1..4, each finite
 * and > 0, strictly increasing), nslot slots (1..32) of N x N cells (N * N < 2^25), connectivity 4 or 8 on the grid
 * (no wrap at the domain edge), one member m with integer weight w >= 1.  For every k and slot, every line a
 * statement of its own:
 *   v(c) = the value ps_summary_add adds for the slot (ps_record_value)
 *   O = {c : v(c) >= t_k}
 *   a patch is a connected component of O; its label is the smallest linear index row * N + col of its cells
 *   the main patch is the patch with the most cells, among equals the one with the smallest label
 *   per member, in add order (uint32 each): npatch;  cells = |O|;  main_cells;  main_label (0xffffffff where O is
 *     empty);  sat_cells_max, the cells of the largest patch that is not the main one, 0 if there is none
 *   main[k][slot][c] += w where c lies in the main patch;  sat[k][slot][c] += w where c is in O outside it
 *   so main + sat is the weighted exceedance count of ps_excur;  an empty O gives an all-zero row (but for the
 *     label) and counts nothing
 * State (pitch as ps_summary): cnt[which][k][slot][pitch] uint32, 2 * K * nslot * pitch * 4 B (184.8 MB at R = 400,
 * 18 days, K = 2); rows[member][k][slot][5] uint32, 20 B per member, threshold and slot, grown by doubling; the
 * weights on the host.  Scratch: parent[k][slot][pitch] and size[k][slot][pitch] uint32 and one 64-bit key per plane
 * -- all K * nslot planes of a member are in flight at once (plane on grid.y), which costs 8 B per cell and plane, as
 * much again as the counts.  Every allocation is checked against the free device memory first: PS_ERR_OOM before it
 * is made.  The labelling is union-find on parent: init (c in O, a NONE value outside), link (each cell of O joined
 * to its occupied left and upper neighbours, with 8-connectivity also the upper-left and upper-right ones; a join is
 * one compare-and-swap on a root, always from the larger root to the smaller, so parent[c] <= c throughout, every
 * loop pass returns or strictly lowers an index and no thread waits for another), flatten (every cell gets its
 * root, the patch's smallest index), sizes (integer adds on size[root] aggregated per wave; npatch and cells), pick
 * (a 64-bit maximum of (size << 32) | (0xffffffff - label) over the roots), count (one writer per cell; the largest
 * size among the other roots).  Integer atomics only and a canonical label: neither the order of adds, nor that of
 * merges, nor the launch configuration, nor the order in which the device joins cells changes a bit; only the order
 * of the members in the fetches follows the adds.  Every operation records an event the next one waits on,
 * whichever stream it runs on (the solver's for add, the handle's own otherwise). */
typedef struct ps_patch ps_patch;
/* PS_ERR_BAD_ARG for thresholds not finite, not > 0, not strictly increasing, more than 4, a connectivity other than
 * 4 or 8, slots outside 1..32 or N * N >= 2^25 */
int ps_patch_create(int device, int N, int nslot, int nthr, const double* thr, int connectivity, ps_patch** out);
/* room for `members` members' rows now (a growth synchronises; never shrinks) */
int ps_patch_reserve(ps_patch* a, int64_t members);
/* One member with weight >= 1 (arguments and refusals as ps_range_add; a total weight past 2^32 - 1 is refused): two
 * small memsets and six launches on the solver's stream, every plane in each; no host synchronisation unless the
 * rows have to grow.  Every descriptor is resolved first, so an add with a bad slot enqueues nothing. */
int ps_patch_add(ps_patch* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                 const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                 uint32_t weight);
/* The same for the current outputs of a projection or a release plan, as ps_range_add_project /
 * ps_range_add_sites: slot e takes Y_e (nslot must equal nout), on the handle's stream. */
int ps_patch_add_project(ps_patch* a, ps_project* p, uint32_t weight);
int ps_patch_add_sites(ps_patch* a, ps_sites* p, uint32_t weight);
/* dst += src: the counts by an integer plane add, src's member rows and weights appended after dst's (a device
 * copy); same device, N, slots, thresholds and connectivity; src unchanged */
int ps_patch_merge(ps_patch* dst, ps_patch* src);
/* any pointer may be NULL; capacity: the members the rows hold room for; bytes: the device memory held now */
int ps_patch_info(ps_patch* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes);
/* zero counts, W and members and drop the timings of ps_patch_prof; the rows keep their room */
int ps_patch_reset(ps_patch* a);
/* (double)cnt[which][k][slot] / (double)W, which 0: the posterior probability that the cell lies in the member's
 * main patch, 1: in O outside it (synchronises).  PS_ERR_STATE before the first add, as the fetches below. */
int ps_patch_prob(ps_patch* a, int k, int slot, int which, double* out /* N*N */);
int ps_patch_fetch_counts(ps_patch* a, int k, int slot, int which, uint32_t* out /* N*N */);
/* per member in add order the row of (k, slot) and the weight (any pointer may be NULL) */
int ps_patch_fetch_members(ps_patch* a, int k, int slot, uint32_t* npatch, uint32_t* cells, uint32_t* main_cells,
                           uint32_t* main_label, uint32_t* sat_cells_max, uint32_t* weights);
/* measurement: HIP-event timing of the adds and the map launches, as ps_range_prof; the totals count from
 * the last ps_patch_reset */
int ps_patch_prof(ps_patch* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps);
void ps_patch_destroy(ps_patch* a);

/* ---- pathway maps: reached by the advancing front or by a jump? ----
 * (no reference counterpart.)  A day kernel is local diffusion plus wind-borne flights, so a member spreads by
 * stratified dispersal (Shigesada, Kawasaki & Takeda 1995): a contiguous patch creeps outward from the release,
 * detached foci are founded downwind, and each grows on its own until the front swallows it.  The arrival maps know
 * a member's first day at a cell but not what the cell was connected to; the patch maps label one day's patches and
 * have no memory of earlier days.  The pairing of "newly reached" with "connected to ground reached before" lives
 * inside one member's sequence of days.  Inputs: the slots s = 0 .. nslot - 1 (1..32) in ascending time, N x N cells
 * each (N * N < 2^25); thresholds t_0 < ... < t_{K-1} (K in 1..4, finite, > 0); connectivity 4 or 8 (no wrap at the
 * domain edge); anchor cells (1..32, on the grid); one member with integer weight w >= 1.  Per threshold t, every line
 * a statement of its own:
 *   v_s(c) = the value ps_summary_add adds for slot s (ps_record_value);  O_s = {c : v_s(c) >= t}
 *   the patches of O_s and their labels are those of ps_patch: connected components, label = smallest linear index
 *   every cell carries a state: 0 unreached, 1 front, 2 jump, 3 secondary; all start at 0
 *   for s = 0, 1, ... in order, with the states as they stood before slot s, for every patch Q of O_s:
 *     origin(Q) = Q holds an anchor, or a cell in state 1
 *     seeded(Q) = Q holds a cell in a non-zero state
 *     every cell of Q still in state 0 becomes 1 if origin(Q), else 3 if seeded(Q), else 2 -- the founding cells of
 *       a new focus, and Q counts as one focus founded in slot s
 *   a state is never changed once set: a focus that merges with the origin patch hands its later cells to the front,
 *     and ground a vanished focus once held seeds secondary growth, not a new focus
 *   after the last slot cnt[k][class][c] += w where the state of c equals the class (0: front, 1: jump, 2: secondary)
 *   rows[member][k][s] = (cells newly classed front, jump, secondary in slot s; foci founded in slot s)
 * so per threshold front + jump + secondary is the arrival count of ps_arrival summed over the slots.
 * State (pitch as ps_summary): cnt[k][3][pitch] uint32; rows[member][k][slot][4] uint32, 16 B per member, threshold
 * and slot, grown by doubling; the weights on the host.  Scratch: parent[k][slot][pitch] and flags[k][slot][pitch]
 * uint32 -- all K * nslot planes of a member are labelled at once (plane on grid.y) -- and state[k][pitch] uint8.
 * bytes = 12 K pitch (counts) + 4 K nslot pitch (parent) + 4 K nslot pitch (flags) + K pitch (states) + 16 K nslot
 * capacity (rows): 201.5 MB at R = 400, 18 days, K = 2.  Every allocation is checked against the free device memory
 * first: PS_ERR_OOM, with the figure, before it is made.  One add: two memsets, init / link / flatten as ps_patch
 * over all planes (ps_patch_core.h), then per slot two launches over the K thresholds -- flag (every cell of O_s
 * whose state is set, and every anchor in O_s, ORs its bits into the flags word at its root, aggregated per wave)
 * and class (one writer per cell; the three classes and the founded roots by ballots, one integer atomic per block
 * and word) -- and one launch that adds w into the count planes.  Nothing a launch writes is read in that launch,
 * but for the link kernel's own atomics.  Integer atomics only and a canonical label: neither the order of adds, nor
 * that of merges, nor the launch configuration, nor the order in which the device joins cells changes a bit; only
 * the order of the members in the fetches follows the adds.  Every operation records an event the next one waits
 * on, whichever stream it runs on (the solver's for add, the handle's own otherwise). */
typedef struct ps_pathway ps_pathway;
/* PS_ERR_BAD_ARG for thresholds not finite, not > 0, not strictly increasing, more than 4, a connectivity other than
 * 4 or 8, slots outside 1..32, anchors outside 1..32 or off the grid, or N * N >= 2^25 */
int ps_pathway_create(int device, int N, int nslot, int nthr, const double* thr, int connectivity, int nanchor,
                      const int32_t* anchor_row, const int32_t* anchor_col, ps_pathway** out);
/* room for `members` members' rows now (a growth synchronises; never shrinks) */
int ps_pathway_reserve(ps_pathway* a, int64_t members);
/* One member with weight >= 1 (arguments and refusals as ps_patch_add; the slots in ascending time): two memsets
 * and 4 + 2 nslot launches on the solver's stream; no host synchronisation unless the rows have to grow.  Every
 * descriptor is resolved first, so an add with a bad slot enqueues nothing. */
int ps_pathway_add(ps_pathway* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                   const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                   uint32_t weight);
/* The same for the current outputs of a release plan, as ps_patch_add_sites: slot e takes Y_e (nslot must equal
 * nout), on the handle's stream. */
int ps_pathway_add_sites(ps_pathway* a, ps_sites* p, uint32_t weight);
/* dst += src: the counts by an integer plane add, src's member rows and weights appended after dst's (a device
 * copy); same device, N, slots, thresholds, connectivity and anchors; src unchanged */
int ps_pathway_merge(ps_pathway* dst, ps_pathway* src);
/* any pointer may be NULL; capacity: the members the rows hold room for; bytes: the device memory held now */
int ps_pathway_info(ps_pathway* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes);
/* zero counts, W and members and drop the timings of ps_pathway_prof; the rows keep their room */
int ps_pathway_reset(ps_pathway* a);
/* cnt[k][which], which 0: front, 1: jump, 2: secondary (synchronises).  PS_ERR_STATE before the first add, as
 * ps_pathway_fetch_members. */
int ps_pathway_fetch_counts(ps_pathway* a, int k, int which, uint32_t* out /* N*N */);
/* per member in add order the row of (k, slot) and the weight (any pointer may be NULL) */
int ps_pathway_fetch_members(ps_pathway* a, int k, int slot, uint32_t* front, uint32_t* jump, uint32_t* secondary,
                             uint32_t* foci, uint32_t* weights);
/* measurement: HIP-event timing of the adds, as ps_summary_prof; the totals count from the last ps_pathway_reset */
int ps_pathway_prof(ps_pathway* a, int enable, double* add_ms, int64_t* adds);
void ps_pathway_destroy(ps_pathway* a);

/* ---- representative members: pairwise overlap of the members' excursion sets ----
 * (no reference counterpart.)  The mean, the quantiles and the excursion sets are maps no member produces.  Which
 * single member is the most typical one, between which two outlines the middle half of the members lies (the contour
 * boxplot of Whitaker, Mirzargar & Kirby 2013) and whether the members fall into a few scenarios depend on how the
 * members' sets relate pairwise, which the count plane has lost.  Setting: one plane (threshold k, slot) of a
 * ps_excur; members m = 0..M-1 in add order, B_m the cells whose mask bit is 1, integer weight w_m >= 1, W = sum w_m.
 * Device:
 *   I[i][j] = |B_i & B_j| as uint32, the full symmetric M x M table, the diagonal n_i = |B_i|; pad bits are 0 in the
 *     masks and do not count
 *   Cs(c) = sum_m s_m bit_m(c) as uint32 for a selection s (uint32 per member, 0: not selected), sum s_m < 2^32 - 1
 * Host (parasitoids_amd/predictive.py, integers only), every line a statement of its own:
 *   out_ij = n_i - I_ij
 *   i is eps-included in j  <=>  1000 out_ij <= e n_i,  e = round(1000 eps), eps a multiple of 0.001 in [0, 0.5]
 *     (Chaves-de-Plaza et al. 2024, the relaxed inclusion); an empty set lies inside every set
 *   in_i = sum_j w_j [i in j];  cont_i = sum_j w_j [j in i], both with j = i;  depth_i = min(in_i, cont_i) in
 *     [w_i, W], reported as depth_i / W
 *   the median member has the largest depth, among equals the smallest index
 *   the central set is the shortest prefix of the members sorted by (-depth, index) whose weight cum satisfies
 *     1000 cum >= c W,  c = round(1000 central), central a multiple of 0.001 in (0, 1]
 *   the band is Cs of the central set with s = w (Wc its weight): +1 where Cs == Wc, 0 where 0 < Cs < Wc, -1 where
 *     Cs == 0
 *   d_ij = n_i + n_j - 2 I_ij, the cells of the symmetric difference
 *   scenarios are weighted k-medoids on d, cost(Med) = sum_i w_i min_{m in Med} d_im, by deterministic PAM (Kaufman
 *     & Rousseeuw): BUILD takes argmin_m sum_i w_i d_im, then the candidate that lowers the cost most, among equals
 *     the smallest index; SWAP takes over every (medoid position, other member) the swap with the largest strict
 *     improvement, among equals the smallest position, then the smallest member, until none improves; a member
 *     goes to its nearest medoid, among equals the one with the smallest index; clusters by descending weight, then
 *     medoid index
 *   the plane 'all' takes I and n summed over the slots in int64
 * State: the handle borrows the ps_excur -- the caller keeps it alive -- and reads its masks, counts and members at
 * every call, so the members present at the call are the members of the answer.  It owns a stream, the M x M table
 * (M * M * 4 B, 25 MB at 2500 members; grown on demand, the free memory checked first: PS_ERR_OOM before it is
 * made), one uint32 plane, the selection vector and two words for the live window.  Every call orders its stream
 * behind the accumulator's last operation and the accumulator's next operation behind its read, and synchronises.
 * The pair kernel works on member tiles of ps_overlap_info's `tile` on or above the diagonal and mirrors when it
 * writes; the word range may be split over workgroups, which then add with integer atomics: neither the grid nor
 * the order changes a bit.  With use_window != 0 it visits only the words from the first to the last one in which
 * the count plane is non-zero (outside them every mask word is zero); the table is the same either way. */
typedef struct ps_overlap ps_overlap;
/* PS_ERR_BAD_ARG unless e is on `device` with domain N */
int ps_overlap_create(int device, int N, ps_excur* e, ps_overlap** out);
/* PS_ERR_STATE while e holds no member; PS_ERR_BAD_ARG for a plane out of range or members_expected != e's members
 * (a caller's buffer is never too small) */
int ps_overlap_pairs(ps_overlap* h, int k, int slot, int64_t members_expected, int use_window,
                     uint32_t* out /* M*M */);
/* sel: `members` entries, NULL for every member with its own weight (Cs is then the count plane); PS_ERR_BAD_ARG
 * for members != e's members or a selection that sums to 2^32 - 1 or more; PS_ERR_STATE while e holds no member */
int ps_overlap_subset(ps_overlap* h, int k, int slot, int64_t members, const uint32_t* sel, uint32_t* out /* N*N */);
/* any pointer may be NULL; members: those of the last pairs call; bytes: the device memory held now; tile: the
 * member-tile edge of the pair kernel */
int ps_overlap_info(ps_overlap* h, int64_t* members, int64_t* bytes, int32_t* tile);
/* measurement: HIP-event timing of the pairs calls (memset, window, pair kernel) and the subset launches, as
 * ps_arrival_prof */
int ps_overlap_prof(ps_overlap* h, int enable, double* pairs_ms, int64_t* pairs_n, double* subset_ms,
                    int64_t* subset_n);
void ps_overlap_destroy(ps_overlap* h);

/* ---- reweighted excursion regions: the excursion functions under one real weight per member ----
 * (no reference counterpart.)  The excursion functions of a ps_excur rest on the members' integer weights.  New
 * findings give every member a real weight (importance reweighting), and everything the functions need is a function
 * of the kept masks and those weights: no member is evaluated again, and the weights may be chosen after the run.
 * Setting: one plane (threshold k, slot) of a ps_excur, members m = 0..M-1 in add order, w_m >= 0 finite, not all 0.
 * Every line is a statement of its own; there is no multiply, so nothing contracts:
 *   W = w_0 + w_1 + ... in add order, from 0.0
 *   C(c) = 0.0, then for m = 0, 1, ...: C += w_m where bit_m(c) is set; one writer per cell
 *   hi_m = max{C(c) : bit_m(c) = 0, c a real cell}, 0.0 if there is none
 *   lo_m = min{C(c) : bit_m(c) = 1}, +inf if the mask is empty
 *   u(c) = min(C, W - C)
 *   above   A+(c) = sum_m w_m [hi_m < C],                  0 where C == 0
 *   below   A-(c) = sum_m w_m [lo_m > C]
 *   contour Ac(c) = sum_m w_m [hi_m < W - u and lo_m > u], 0 where u + u >= W
 *   each sum over the members in add order from 0.0; every map is A / W, one division; prob is C / W
 * A member of weight 0 keeps its mask and its bounds and adds 0.  Non-negative doubles order like their bit
 * patterns: the bounds are integer maxima and minima of 64-bit words, so no order of waves changes a bit.  With
 * w_m the integer weights of the members, C, hi, lo (its "none" as +inf) and the three maps are those of the
 * ps_excur, bit for bit.
 * State: the handle borrows the ps_excur -- the caller keeps it alive -- and owns a stream, two fp64 planes of the
 * pitch (C and the map scratch) and 3 x members x 8 B (hi, lo, w; grown on demand, the free memory checked first).
 * It keeps one current plane: the maps and fetches answer for it, and are refused (PS_ERR_STATE) once the ps_excur
 * holds other members than when the plane was formed. */
#define PS_WEXCUR_ABOVE 0
#define PS_WEXCUR_BELOW 1
#define PS_WEXCUR_CONTOUR 2
#define PS_WEXCUR_PROB 3
typedef struct ps_wexcur ps_wexcur;
/* PS_ERR_BAD_ARG unless e is on `device` with domain N */
int ps_wexcur_create(int device, int N, ps_excur* e, ps_wexcur** out);
/* forms C and the bounds of plane (k, slot) under w[members] and keeps them as the current plane (synchronises).
 * Refused, enqueuing nothing and keeping the current plane: PS_ERR_BAD_ARG for a plane out of range, members != e's
 * members, a weight that is negative or not finite, or weights that are all 0; PS_ERR_STATE while e holds no member */
int ps_wexcur_plane(ps_wexcur* h, int k, int slot, int64_t members, const double* w);
int ps_wexcur_fetch_counts(ps_wexcur* h, double* out /* N*N */);
/* either pointer may be NULL */
int ps_wexcur_fetch_bounds(ps_wexcur* h, double* hi /* members */, double* lo /* members */);
/* what = PS_WEXCUR_ABOVE / _BELOW / _CONTOUR / _PROB of the current plane (synchronises) */
int ps_wexcur_map(ps_wexcur* h, int what, double* out /* N*N */);
/* any pointer may be NULL; members and total_weight (W): of the current plane, 0 without one; bytes: the device
 * memory held now */
int ps_wexcur_info(ps_wexcur* h, int64_t* members, int64_t* bytes, double* total_weight);
/* the integer weights the members of e were added with, in add order; PS_ERR_BAD_ARG for members != e's members */
int ps_wexcur_member_weights(ps_wexcur* h, int64_t members, uint32_t* out /* members */);
/* measurement: HIP-event timing of the count launches [0], the bounds [1] and the maps [2], as ps_excur_prof */
int ps_wexcur_prof(ps_wexcur* h, int enable, double* ms /* 3 */, int64_t* launches /* 3 */);
void ps_wexcur_destroy(ps_wexcur* h);

/* ---- neighbourhood fields: the largest value of one member's field within r of each cell ----
 * (no reference counterpart; the neighbourhood maximum of Schwartz & Sobash 2017, whose ensemble statistics the
 * accumulators below then take.)  A handle lives on one device and holds nout outputs (1..32) over nin inputs
 * (1..32): output e is (input[e], r2[e]) with 0 <= input[e] < nin and r2[e] a whole squared radius in cells with
 * H = floor(sqrt(r2[e])) <= PS_NBHD_MAX_HALF = 32, i.e. 0 <= r2[e] <= 1088 (PS_ERR_BAD_ARG otherwise), and nout fp64
 * fields Z[e][pitch] (pitch as ps_summary).  With v the value of input[e], an apply overwrites every cell of every
 * output, zeros included, with
 *   Z_e(y, x) = max { v(y', x') : 0 <= y', x' < N,  (y' - y)^2 + (x' - x)^2 <= r2[e] }.
 * Cells outside the domain do not exist: nothing wraps and no padding value takes part.  r2 = 0 gives Z = v.  A
 * maximum is exact, so Z is the same whatever the tile, the launch shape or the order of the comparisons.
 * The disc is a stack of horizontal chords of half-width w(dy) = floor(sqrt(r2 - dy^2)), |dy| <= H; the maximum
 * over a chord clipped to the domain, len cells from column a, is max(L_k(a), L_k(a + len - 2^k)) with
 * k = floor(log2(len)) and L_k(y, x) = max v(y, x .. x + 2^k - 1).  One workgroup owns a tile of 32 x 64 cells of
 * one input and up to 8 of the outputs that read it (the outputs are grouped by input): it stages v of the tile
 * and a halo of the largest H among them -- only the cells of the domain -- in LDS ((32 + 2H)(64 + 2H) 8 B, 98304 B
 * at H = 32), folds at every level k the chords of that level into register accumulators that start from the
 * centre cell, and doubles the windows in place between two barriers.  Work per cell grows like H, not H^2.  One
 * writer per cell, no atomics.  Unless switched off (ps_nbhd_set_skip), a pre-pass writes per input and tile
 * whether the tile holds a value != 0, and a tile whose own and eight neighbouring tiles are all empty stores zeros
 * without staging; the outputs are the same either way.  The handle holds nout * pitch * 8 B and nin int32 flags
 * per tile (nin * ceil(N / 32) * ceil(N / 64) * 4 B), checked against the free device memory first: PS_ERR_OOM
 * before anything is allocated.  Every operation records an event the next one waits on, whichever stream it runs
 * on (the solver's for ps_nbhd_apply, the handle's own for the other applies, fetch and gather, the accumulator's
 * for the _add_nbhd entry points). */
#define PS_NBHD_MAX_HALF 32
typedef struct ps_nbhd ps_nbhd;
int ps_nbhd_create(int device, int N, int nin, int nout, const int32_t* input /* nout */,
                   const int32_t* r2 /* nout */, ps_nbhd** out);
/* on != 0 (the default): the empty-tile pre-pass; 0: every tile is staged.  Takes effect at the next apply. */
int ps_nbhd_set_skip(ps_nbhd* c, int on);
/* The inputs are records of solver s (same device, same N; arguments as ps_catch_apply, nin must equal the
 * handle's; v is the value ps_summary_add adds, bit for bit): on the solver's stream, no host synchronisation,
 * nothing copied or allocated.  Every descriptor is resolved before anything is enqueued. */
int ps_nbhd_apply(ps_nbhd* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                  const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* The inputs are the current outputs of a projection or a release plan: input i is the source's output i, so
 * nin must equal its nout, and device and N must agree (PS_ERR_BAD_ARG, nothing enqueued); PS_ERR_STATE before
 * the source's first apply.  On the handle's stream behind the source's last operation; the source's next apply
 * waits for the read. */
int ps_nbhd_apply_project(ps_nbhd* c, ps_project* p);
int ps_nbhd_apply_sites(ps_nbhd* c, ps_sites* p);
/* one output field to the host (synchronises).  PS_ERR_STATE before the first apply. */
int ps_nbhd_fetch(ps_nbhd* c, int e, double* out /* N*N */);
/* the outputs at n listed cells: out[e * n + k] = Z_e(rows[k], cols[k]) (synchronises).  PS_ERR_BAD_ARG for
 * a cell outside the domain, PS_ERR_STATE before the first apply. */
int ps_nbhd_gather(ps_nbhd* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out /* nout x n */);
/* any pointer may be NULL */
int ps_nbhd_info(ps_nbhd* c, int* N, int* nin, int* nout, int64_t* applies);
/* measurement: HIP-event timing of the applies (pre-pass and transform together), as ps_catch_prof */
int ps_nbhd_prof(ps_nbhd* c, int enable, double* total_ms, int64_t* launches);
void ps_nbhd_destroy(ps_nbhd* c);
/* One member whose values are the handle's current outputs, as ps_summary_add_catch takes a catch handle's: slot
 * e takes Z_e, through the accumulator's own add kernel, on the accumulator's stream behind the handle's last
 * operation; the next apply waits for the read.  The accumulator's slot count must equal nout, device and N must
 * agree (PS_ERR_BAD_ARG, nothing enqueued); PS_ERR_STATE before the first apply. */
int ps_summary_add_nbhd(ps_summary* a, ps_nbhd* c, uint32_t weight);
int ps_hist_add_nbhd(ps_hist* h, ps_nbhd* c, uint32_t weight);
int ps_mcerr_add_nbhd(ps_mcerr* h, ps_nbhd* c, uint32_t weight);
int ps_wsum_add_nbhd(ps_wsum* h, ps_nbhd* c, int nscen, const double* rescale, const double* omega);

/* ---- ensemble modes: the weighted principal components of the members' fields ----
 * (no reference counterpart; the EOFs of ensemble forecasting, and with the square root the Hellinger-type PCA of
 * Legendre & Gallagher 2001.)  The spread map says how much the members differ at a cell, not which cells vary
 * together.  That needs the inner product of every pair of members' real-valued fields, which no accumulator keeps.
 * A handle lives on one device and holds, for N x N cells and nslot day slots (1..8, ascending), the members'
 * transformed fields X[member][slot][pitch] as fp64 (pitch as ps_summary, the pad cells 0) in add order, and on the
 * host an integer weight w_m >= 1 per member, W = sum w_m < 2^32 - 1.  With v the value ps_summary_add adds for the
 * slot (>= 0), X = v (PS_MODES_RAW) or X = sqrt(v), the IEEE round-to-nearest square root (PS_MODES_SQRT).  Per slot:
 *   mu(c)   = (sum_m w_m X_m(c)) / W: acc = acc + w_m * X_m(c) over m in add order, the product and the sum each
 *             rounded once, then one division -- bit for bit the numpy loop acc += w * X[m]; acc / W
 *   A_m     = X_m - mu (centred, one IEEE subtraction per cell) or X_m
 *   G_ij    = sum_c A_i(c) A_j(c), the full symmetric M x M table
 *   out_k(c) = sum_m coef_km A_m(c) over m in add order, product and sum rounded separately: bit for bit a numpy loop
 * The table is a symmetric fp64 product on the matrix units (v_mfma_f64_16x16x4_f64): a workgroup owns a pair of
 * 64-member tiles on or above the diagonal and a share of the cell axis, stages both tiles through LDS (the mean
 * subtracted, members past M and cells past the range zeroed) and mirrors when it writes.  The splits of the cell
 * axis -- their number depends on M and N only -- write partial tables that a second kernel adds in split order: no
 * floating-point atomics, two calls on one handle return the same bits, and G is symmetric to the bit.  Any summation
 * order satisfies |G_ij - exact| <= gamma_P sqrt(G_ii G_jj), P = N * N.  Unless switched off (ps_modes_set_window) the
 * table visits only the cells from the first to the last word of 64 cells in which mu != 0: outside them every X_m is
 * 0 (X >= 0, w >= 1), so the terms left out are zeros, though the splits then fall elsewhere and the last bits may
 * differ from the unwindowed table.  The eigen-decomposition is the host's (parasitoids_amd/predictive.py,
 * mode_decomposition).  The handle holds cap * nslot * pitch * 8 B of fields (5.13 MB per member and slot at N = 801),
 * nslot mean planes, the partial tables and, after the first combine, 8 planes; every allocation is checked against
 * the free device memory first: PS_ERR_OOM before it is made.  The fields grow by doubling (copied, never shrunk).
 * Every operation records an event the next one waits on, whichever stream it runs on (the solver's for ps_modes_add,
 * the handle's own for everything else). */
#define PS_MODES_RAW 0
#define PS_MODES_SQRT 1
typedef struct ps_modes ps_modes;
/* PS_ERR_BAD_ARG for slots outside 1..8 or a transform that is neither PS_MODES_RAW nor PS_MODES_SQRT */
int ps_modes_create(int device, int N, int nslot, int transform, ps_modes** out);
/* room for `members` members now (exactly; PS_ERR_OOM with nothing allocated if the device has not that much free) */
int ps_modes_reserve(ps_modes* a, int64_t members);
/* on != 0 (the default): the table visits the live window only; 0: the whole plane */
int ps_modes_set_window(ps_modes* a, int on);
/* One member from records of solver s with the arguments and refusals of ps_excur_add: one launch on the solver's
 * stream, every cell of every slot of the member written, zeros and pad included; weight >= 1. */
int ps_modes_add(ps_modes* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                 const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                 uint32_t weight);
/* One member whose slots are the current outputs of a projection or a release plan, as ps_excur_add_project. */
int ps_modes_add_project(ps_modes* a, ps_project* p, uint32_t weight);
int ps_modes_add_sites(ps_modes* a, ps_sites* p, uint32_t weight);
/* One member from host arrays v[nslot][N*N]; the transform is applied.  A negative or non-finite value is
 * PS_ERR_BAD_ARG with nothing stored (synchronises). */
int ps_modes_add_host(ps_modes* a, const double* fields /* nslot x N*N */, uint32_t weight);
/* dst's members, then src's, by a device copy; device, N, slots and transform must match (PS_ERR_BAD_ARG); src is
 * unchanged */
int ps_modes_merge(ps_modes* dst, ps_modes* src);
/* any pointer may be NULL; capacity: the members the fields hold room for; bytes: the device memory held now */
int ps_modes_info(ps_modes* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes);
/* the members' weights in add order; PS_ERR_BAD_ARG for members_expected != the handle's members */
int ps_modes_weights(ps_modes* a, int64_t members_expected, uint32_t* out /* members */);
/* forget every member (the room stays) */
int ps_modes_reset(ps_modes* a);
/* mu of one slot (synchronises); the plane stays on the device until the next add, merge or reset.  PS_ERR_STATE
 * before the first add, as table, combine and fetch_member. */
int ps_modes_mean(ps_modes* a, int slot, double* out /* N*N */);
/* G of one slot (synchronises).  PS_ERR_BAD_ARG for members_expected != the handle's members (a caller's buffer is
 * never too small). */
int ps_modes_table(ps_modes* a, int slot, int centred, int64_t members_expected, double* out /* M*M */);
/* ncoef (1..8) linear combinations of the members' (centred) fields, the members read once for all of them
 * (synchronises) */
int ps_modes_combine(ps_modes* a, int slot, int centred, int ncoef, const double* coef /* ncoef x M */,
                     double* out /* ncoef x N*N */);
/* the stored X of one member (synchronises) */
int ps_modes_fetch_member(ps_modes* a, int64_t member, int slot, double* out /* N*N */);
/* measurement: HIP-event timing of 0 the adds, 1 the mean launches, 2 the table calls (window, product, sum of the
 * splits) and 3 the combine launches, as ps_excur_prof */
int ps_modes_prof(ps_modes* a, int enable, double* ms /* 4 */, int64_t* launches /* 4 */);
void ps_modes_destroy(ps_modes* a);

/* ---- proximity fields: how far from each cell is the nearest ground that holds t wasps ----
 * (no reference counterpart; the exact Euclidean distance transform of Danielsson 1980 in the two-pass form of
 * Meijster, Roerdink & Hesselink 2000, whose ensemble statistics the accumulators below then take.)  A handle lives
 * on one device and holds nout outputs (1..32) over nin inputs (1..32) on a domain of N <= 32767 cells a side, so
 * that every squared distance fits 32 bits (PS_ERR_BAD_ARG otherwise): output e is (input[e], thr[e], side[e]) with
 * 0 <= input[e] < nin, thr[e] not a NaN and side[e] 0 or 1; cell_m > 0 and finite.  With v the value of input[e]
 * and S = {(y, x) : 0 <= y, x < N, v(y, x) >= thr[e]}, an apply overwrites every cell of every output with
 *   side 0 ("to"):  d2_e(y, x) = min { (y - y')^2 + (x - x')^2 : (y', x') in S }, 0 on S
 *   side 1 ("in"):  the same with S replaced by its complement within the domain: the depth of a reached cell
 *                   inside the reached ground, 0 off S
 *   where the set searched for is empty: d2 = far2 = 2 (N - 1)^2 + 1, one more than the domain can hold
 *   Z_e(y, x) = fl(fl(sqrt((double) d2)) * cell_m), in metres; the IEEE round-to-nearest square root
 * Nothing wraps; cells outside the domain do not exist and the domain's edge is not unreached ground.  d2 is an
 * exact integer, so both planes are the same whatever the strip, the launch shape or the order of the search.
 * Three launches.  The set as 64-bit words, bit c & 63 of word c >> 6 for cell c = y N + x (pitch / 64 words per
 * output, the layout of ps_excur): one thread per cell, one ballot per wave.  The row pass: one thread per cell
 * takes g(y, x), the distance along its own row to the nearest set bit, from the leading and trailing zeros of its
 * own word and a walk over the row's words outwards; uint16, 0xffff where the row holds none.  The column pass:
 * d2(y, x) = min over y' of (y - y')^2 + g(y', x)^2; a workgroup owns a strip of W columns of one output and a share
 * of its rows, stages g of the whole strip in LDS (W N 2 B: 102528 B at N = 801) and every thread searches
 * dy = 0, 1, 2, .. on both sides until dy^2 >= its best, so the work per cell grows like its distance; d2 and Z are
 * written in the same pass.  W is the widest power of two <= 64 with W N 2 B <= the LDS one workgroup may hold
 * (at 160 KiB: 64 up to N = 1280, 32 up to 2560, 16 up to 5120, .., 2 up to 32767); the rows of a strip are shared
 * among floor(CUs / (strips x nout)) workgroups, 1..64.  One writer per cell, no atomics, no hand-off between
 * workgroups.  The handle holds nout * pitch * (8 + 4 + 2 + 1/8) B (Z, d2, g, the words), checked against the free
 * device memory first: PS_ERR_OOM before anything is allocated.  Every operation records an event the next one waits
 * on, whichever stream it runs on (the solver's for ps_prox_apply, the handle's own for the other applies, fetch and
 * gather, the accumulator's for the _add_prox entry points). */
typedef struct ps_prox ps_prox;
int ps_prox_create(int device, int N, int nin, int nout, const int32_t* input /* nout */,
                   const double* thr /* nout */, const int32_t* side /* nout */, double cell_m, ps_prox** out);
/* testing: the strip of the next applies, a power of two <= the default; 0: the default.  PS_ERR_BAD_ARG otherwise.
 * The outputs are the same. */
int ps_prox_set_strip(ps_prox* c, int width);
/* The inputs are records of solver s, with the arguments and refusals of ps_nbhd_apply: on the solver's stream, no
 * host synchronisation, nothing copied or allocated.  Every descriptor is resolved before anything is enqueued. */
int ps_prox_apply(ps_prox* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                  const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* The inputs are the current outputs of a projection or a release plan, as ps_nbhd_apply_project. */
int ps_prox_apply_project(ps_prox* c, ps_project* p);
int ps_prox_apply_sites(ps_prox* c, ps_sites* p);
/* one output to the host, in metres or as the squared distance in cells (synchronises).  PS_ERR_STATE before the
 * first apply. */
int ps_prox_fetch(ps_prox* c, int e, double* out /* N*N */);
int ps_prox_fetch_d2(ps_prox* c, int e, uint32_t* out /* N*N */);
/* the outputs at n listed cells: out[e * n + k] = Z_e(rows[k], cols[k]) (synchronises).  PS_ERR_BAD_ARG for
 * a cell outside the domain, PS_ERR_STATE before the first apply. */
int ps_prox_gather(ps_prox* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out /* nout x n */);
/* any pointer may be NULL; strip: the width W in use */
int ps_prox_info(ps_prox* c, int* N, int* nin, int* nout, int64_t* applies, int* strip);
/* measurement: HIP-event timing of the applies, the set and the row pass apart from the column pass (an event
 * pair each); both counts are the applies timed */
int ps_prox_prof(ps_prox* c, int enable, double* row_ms, int64_t* row_n, double* col_ms, int64_t* col_n);
void ps_prox_destroy(ps_prox* c);
/* One member whose values are the handle's current outputs in metres, as ps_summary_add_nbhd takes a
 * neighbourhood handle's. */
int ps_summary_add_prox(ps_summary* a, ps_prox* c, uint32_t weight);
int ps_hist_add_prox(ps_hist* h, ps_prox* c, uint32_t weight);
int ps_mcerr_add_prox(ps_mcerr* h, ps_prox* c, uint32_t weight);
int ps_wsum_add_prox(ps_wsum* h, ps_prox* c, int nscen, const double* rescale, const double* omega);

/* ---- origin maps: from where, when and in what number did the wasps in these traps start ----
 * (no reference counterpart; Bayesian source-term estimation by exhaustive evaluation over every candidate cell,
 * the parameter uncertainty integrated out over the members.)  Inference about an unknown of the past: it
 * recommends nothing and chooses no plan.  Statement by statement, with N = 2 R + 1 odd:
 *   findings   o = 0 .. O - 1, 1 <= O <= 64: cell (row_o, col_o) inside the domain, day slot slot_o in 0 .. nslot - 1
 *              (the distinct calendar days of the findings, 1 <= nslot <= 32), kind_o 0 'count' / 1 'none' / 2 'found',
 *              rate_o finite and > 0, n_o a whole number >= 0 ('count' only)
 *   hypotheses h = 0 .. H - 1, 1 <= H <= 8: amount_h finite and > 0 in multiples of the release number, and the
 *              group hgroup_h in 0 .. ngroup - 1 of its release day (1 <= ngroup <= 4, every group with at least one
 *              hypothesis); a group is one lag, as in ps_sites, and the handle never sees the lag itself: the
 *              caller's slots of group g name model day d - lag_g of that lag's solver, or PS_REC_NONE where d < lag_g
 *   field      for the candidate origin s = (r, c): v = V_slot(row_o + R - r, col_o + R - c), V the value
 *              ps_summary_add adds for the slot's record (ps_record_value: same arguments, same bits); v = 0 where
 *              the source row or the source column leaves [0, N) -- nothing wraps -- and v = 0 under PS_REC_NONE
 *   mu         = ra * v with ra = rate_o * amount_h, one fp64 product formed on the host at create
 *   term       'none', and 'count' with n = 0: -mu.  Otherwise -inf at mu = 0, and at mu > 0
 *              'count': n log(mu) - mu - lgamma(n + 1), the lgamma a host constant per finding;
 *              'found': log(-expm1(-mu)) up to mu = log 2, log1p(-exp(-mu)) above it
 *   l_h(s)     the sum of the terms from +0.0 in the kernel's order, fixed at create: the findings that can give
 *              -inf ('found', 'count' with n > 0) first, each class in the order given.  -inf once a term is -inf.
 *              Compared with a reference within a bound, not bit for bit: log, exp, expm1 and log1p
 *              are the device library's.  The set {l = -inf} is exact.
 *   prior      an optional plane log pi of N * N fp64, finite or -inf (NaN, +inf: PS_ERR_BAD_ARG), NULL: zeros.
 *              A cell at -inf gathers nothing, its l is -inf and it never becomes finite.
 *   (A, S)     per hypothesis and cell, fp64, (-inf, 0) after create and reset.  A member of weight w with l = x:
 *              x = -inf: nothing;  A = -inf: A = x, S = w;  x <= A: S = S + w exp(x - A);
 *              otherwise S = S exp(A - x) + w, A = x.  merge applies the same rule with (x, w) = the other
 *              handle's (A, S).  E_h(s) = A + log S - log W is the caller's, W the total weight.
 *   rows       per member and hypothesis (mx, sum): mx = max over s of l + log pi, sum = sum over s of
 *              exp(l + log pi - mx); (-inf, 0) where no cell is finite.  Two stages: every block of 256 cells
 *              leaves (max, sum) of its own cells, its four waves added in wave order after a butterfly within
 *              the wave; one wave per hypothesis then takes the maximum of the partials, lane k adds
 *              sum_b exp(max_b - mx) over its ceil(nblk / 64) consecutive partials in index order, and lane 0 adds
 *              the 64 lane sums in lane order.  No floating-point atomics: the same calls give the same bits.
 * One writer per cell, no atomics.  The accumulator is floating point, unlike the integer maps: another order of
 * adds or merges moves E within the bound of DESIGN 7y, and changes no -inf.  Memory: 3 H pitch 8 B (A, S, the last
 * member's l), the prior plane where given, H ceil(N N / 256) 16 B of partials, the tables, and the member rows
 * (H 16 B each, grown by doubling from 64), checked against the free device memory before anything is allocated:
 * PS_ERR_OOM.  Every operation records an event the next one waits on, whichever stream it runs on; add does
 * not synchronise the host unless the rows grow. */
typedef struct ps_origin ps_origin;
int ps_origin_create(int device, int N, int nfind, const int32_t* row /* nfind */, const int32_t* col /* nfind */,
                     const int32_t* slot /* nfind */, const int32_t* kind /* nfind */, const double* rate /* nfind */,
                     const double* n /* nfind */, int nslot, int nhyp, const double* amount /* nhyp */,
                     const int32_t* hgroup /* nhyp */, int ngroup, const double* log_prior /* N*N or NULL */,
                     ps_origin** out);
/* room for `members` member rows now, so that no add has to grow them */
int ps_origin_reserve(ps_origin* p, int64_t members);
/* One group of one member from the records of solver s, on the solver's stream: the arguments of ps_sites_apply,
 * one slot per distinct day, PS_REC_NONE included (a group whose every slot is PS_REC_NONE: PS_ERR_BAD_ARG), and
 * the member's integer weight >= 1, the same for every group of the member.  Groups come 0 .. ngroup - 1 in
 * order, any other order is PS_ERR_STATE -- group 0 may not come early, since the groups already in have changed
 * (A, S).  The launch computes l of the group's hypotheses, updates their (A, S) and leaves their rows; the member
 * counts once its last group is in.  Every descriptor is resolved before anything is enqueued. */
int ps_origin_add(ps_origin* p, ps_solver* s, int group, int nslot, const int32_t* kind, const int32_t* idx,
                  const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                  uint32_t weight);
/* dst takes src's (A, S) by the rule above and appends src's rows and weights; src is unchanged.  Device, N,
 * findings, hypotheses, slots and the presence of a prior must agree (PS_ERR_BAD_ARG); PS_ERR_STATE while either
 * handle has a member under way. */
int ps_origin_merge(ps_origin* dst, ps_origin* src);
/* (A, S) back to (-inf, 0), W, the members and a member under way dropped */
int ps_origin_reset(ps_origin* p);
/* one plane of hypothesis h to the host (synchronises): what 0 A, 1 S, 2 the last member's l.  PS_ERR_STATE before
 * the first member and while a member is under way. */
int ps_origin_fetch(ps_origin* p, int what, int h, double* out /* N*N */);
/* the members' rows [members][nhyp][2] and weights in add order (either may be NULL; synchronises); PS_ERR_BAD_ARG
 * for members_expected != the handle's members */
int ps_origin_members(ps_origin* p, int64_t members_expected, double* rows, uint32_t* weights);
/* any pointer may be NULL; bytes: the device memory the handle holds now */
int ps_origin_info(ps_origin* p, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes);
/* measurement: HIP-event timing per kernel class: the likelihood-and-accumulate launches, the row reductions, the
 * merges */
int ps_origin_prof(ps_origin* p, int enable, double* add_ms, int64_t* adds, double* rows_ms, int64_t* rows_n,
                   double* merge_ms, int64_t* merges);
void ps_origin_destroy(ps_origin* p);

/* ---- origin maps over a known release in the background: is there a second source? ----
 * The findings also catch the wasps of releases that are facts, not hypotheses -- ours at the centre.  There is
 * still one unknown origin, evaluated exhaustively; this is no multi-source inversion.  A handle without known
 * releases behaves and computes as above, bit for bit.  Statement by statement:
 *   known releases  k = 0 .. K - 1, 1 <= K <= 32: amount_k finite and > 0 in multiples of the release number, the
 *              cell offset (drow_k, dcol_k) off the centre by the package's convention (|drow|, |dcol| <= N - 1),
 *              and the known group kgroup_k in 0 .. nk - 1 of its lag (1 <= nk <= 4, ascending lag, the smallest 0,
 *              every group with at least one release).  The known groups are numbered apart from the hypotheses'.
 *   background per member and finding o: bg_o = the sum over k in index order, from +0.0, of
 *              fl(fl(rate_o * amount_k) * v_k): the bracket formed once on the host at set-up, the product and the
 *              sum rounded separately.  v_k is ps_record_value of the known lag's own model, with the arguments
 *              ps_origin_add takes, read at day d_o - lag_k and cell (row_o - drow_k, col_o - dcol_k); 0 where
 *              either axis leaves [0, N) -- per axis, never by the flat index -- and 0 before that release
 *              (PS_REC_NONE).  A numpy loop gives the same bits.
 *   likelihood for candidate s and hypothesis h: t = ra * v as above, then mu = bg_q + t -- two statements, two
 *              roundings -- then the term above at mu, unchanged.  A finding excludes a cell only where bg_q == 0
 *              and v == 0.  The order of the findings, (A, S), the partials and the rows are unchanged; mu is the
 *              same fp64 number on the device and in the restatement, so the bounds of DESIGN 7y stand as written.
 *   null row   per member l0 = the sum over q, from +0.0 in the kernel's order, of the term at mu = bg_q: "the
 *              known releases alone".  One fixed-order sum of at most 64 terms, kept per member next to the
 *              member rows in add order; its bound is that of l with O terms.
 *   identity   at a candidate cell whose shifted reads are all 0 (and that the prior does not mask),
 *              l_h(s) == l0 bit for bit.
 * One member: ps_origin_background for known group 0 .. nk - 1 in order, then ps_origin_add for group
 * 0 .. ngroup - 1 as above.  Each background call is one small launch on that lag's solver stream -- lane o owns
 * finding o and walks the group's releases in index order; the last known group's launch also adds the terms to
 * bg and forms l0, which one lane sums -- ordered against every other operation of the handle through its
 * last-operation event, without a host synchronisation. */
/* once, before the first member (PS_ERR_STATE afterwards, and for a second call); validated as ps_origin_create
 * validates, each refusal with its offender named */
int ps_origin_set_known(ps_origin* p, int nknown, const int32_t* drow /* nknown */, const int32_t* dcol /* nknown */,
                        const double* amount /* nknown */, const int32_t* kgroup /* nknown */, int nkgroup);
/* One known group of one member from the records of solver s (the arguments of ps_origin_add without the weight;
 * a known group released after every finding may have every slot PS_REC_NONE and contributes 0).  PS_ERR_STATE
 * for a handle without known releases, a call out of order, and a call while the adds of a member are under way.
 * With known releases ps_origin_add(group 0) is PS_ERR_STATE until the member's backgrounds are complete. */
int ps_origin_background(ps_origin* p, ps_solver* s, int kgroup, int nslot, const int32_t* kind, const int32_t* idx,
                         const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval);
/* the bg [nfind] of the last member added to this handle, in the order the findings were given, and its l0 (either
 * may be NULL; synchronises; a merge appends null rows and leaves this pair alone).
 * PS_ERR_STATE without known releases, before the first member and while a member is under way. */
int ps_origin_fetch_background(ps_origin* p, double* bg /* nfind */, double* l0);
/* the members' l0 [members] in add order (synchronises); PS_ERR_STATE without known releases, PS_ERR_BAD_ARG for
 * members_expected != the handle's members.  merge requires equal known releases (PS_ERR_BAD_ARG) and appends the
 * null rows; reset, reserve and the growth of the rows carry them along; info's bytes include them. */
int ps_origin_null_rows(ps_origin* p, int64_t members_expected, double* rows /* members */);

/* ---- reweighted paired contrast: is plan A still better than plan B under new observations? ----
 * (no reference counterpart.)  ps_contrast's maps of d = a - b with the real weights of ps_wsum: J scenarios
 * (1..4), nslot slots (1..32) of N x N cells and K thresholds (0..4, each finite and > 0, strictly increasing).
 * a and b are the fields two ps_sites or two ps_project hold for the same member, so the pairing, which the
 * reweighted maps of either plan alone have lost, is kept.  Per scenario j on the device, all fp64 (pitch as
 * ps_summary; P = 2 + 2 K):
 *   mean[j][slot][pitch], m2[j][slot][pitch], S[j][slot][P][pitch]
 * with the planes of S in the order pos (d > 0), neg (d < 0), gain_0 (a >= t_0 > b), loss_0 (b >= t_0 > a),
 * gain_1, ..., and on the host W_j (a double, 0 while empty), members_j and skipped_j.  The whole block,
 * J * (4 + 2 K) * 8 B * nslot * pitch, is checked against the free device memory first: PS_ERR_OOM before
 * anything is allocated.  At R = 400 (N = 801, pitch 641 664), 18 output days and K = 2 one scenario takes
 * 641 664 x 18 x 64 B = 739 MB.  The per-member coverage rows are not kept here: they are those of the
 * ps_contrast fed alongside.  One thread owns a pair of cells: no atomics, the same calls in the same order
 * give the same bits.  Every operation runs on the handle's stream behind its last one. */
typedef struct ps_wcontrast ps_wcontrast;
/* PS_ERR_BAD_ARG (and *out = NULL) for nscen outside 1..4, nslot outside 1..32, nthr outside 0..4 or thresholds
 * that are not finite, > 0 and strictly increasing */
int ps_wcontrast_create(int device, int N, int nscen, int nslot, int nthr, const double* thr, ps_wcontrast** out);
/* One member from the last apply of a and b, as ps_contrast_add_sites / _add_project take them: slot e takes
 * a = Y_e of a and b = Y_e of b.  rescale[nscen] (r, in [0, 1]) and omega[nscen] (>= 0, finite) as ps_wsum_add;
 * omega_j == 0: the member leaves scenario j untouched and skipped_j grows by one.  For a scenario with
 * omega > 0, every step a statement of its own (one rounding each, but for the two statements of
 * ps_summary_add, which contract as they do there):
 *   host:      W = W * r;  W = W + omega;
 *   per cell:  d = a - b (once, for every scenario);  q = q * r;  S_p = S_p * r (every plane);  e = d - m;
 *              e != 0:  m += e omega / W,  q += omega e (d - m)        (the statements of ps_summary_add)
 *              d > 0: S_pos = S_pos + omega;   d < 0: S_neg = S_neg + omega;
 *              a >= t_k and b < t_k: S_gain_k = S_gain_k + omega;   b >= t_k and a < t_k: S_loss_k = S_loss_k + omega
 * so with r = 1 and integer omega the handle holds the mean and M2 of a ps_contrast fed alongside bit for bit,
 * and its sums are that handle's counts.  A value is stored only where its bits changed, and with r == 1 a pair
 * of cells with d == 0 against a mean of 0 reads its means alone.  An add moves, per slot and cell, 16 B of a
 * and b and per scenario that takes the member 8 B of mean; where something can change, 16 + 16 P B more, read
 * and written.  One launch per member on the handle's stream behind both sources' last operation, no host
 * synchronisation; their next apply waits for the read.  PS_ERR_BAD_ARG (everything is checked before anything
 * is enqueued; a refused add changes nothing): a == b, a source with other outputs than the handle's slots or of
 * another device or domain, a wrong nscen, r outside [0, 1], omega NaN, negative or infinite. */
int ps_wcontrast_add_sites(ps_wcontrast* h, ps_sites* a, ps_sites* b, int nscen, const double* rescale,
                           const double* omega);
int ps_wcontrast_add_project(ps_wcontrast* h, ps_project* a, ps_project* b, int nscen, const double* rescale,
                             const double* omega);
/* dst += src per scenario, same device, N, scenarios, slots and thresholds; src stays as it is.  The rule and
 * the expressions of ps_wsum_merge: Wa' = Wa ra, Wb' = Wb rb, W = Wa' + Wb',
 *   e = mean_b - mean_a;  mean = mean_a + e (Wb' / W);  m2 = m2a ra + m2b rb + e^2 (Wa' Wb' / W);  S = Sa ra + Sb rb.
 * A scenario empty in src adds its skipped count alone; into a scenario empty in dst it is a device copy, bit
 * for bit, W included (ra, rb unused). */
int ps_wcontrast_merge(ps_wcontrast* dst, ps_wcontrast* src, const double* ra, const double* rb);
/* per scenario (any pointer may be NULL): W, members (adds with omega > 0) and skipped (adds with omega == 0) */
int ps_wcontrast_info(ps_wcontrast* h, double* total_weight /* nscen */, int64_t* members, int64_t* skipped);
/* one slot of one scenario to the host (synchronises): what 0 mean, 1 variance m2 / W, 2 P(d > 0), 3 P(d < 0),
 * 4 + 2k gain_k, 5 + 2k loss_k, each probability min(S / W, 1.0).  PS_ERR_STATE while the scenario has W = 0. */
int ps_wcontrast_fetch(ps_wcontrast* h, int scen, int slot, int what, double* out /* N*N */);
int ps_wcontrast_reset(ps_wcontrast* h);
/* measurement: HIP-event timing of the add launches, as ps_summary_prof */
int ps_wcontrast_prof(ps_wcontrast* h, int enable, double* total_ms, int64_t* launches);
void ps_wcontrast_destroy(ps_wcontrast* h);

#ifdef __cplusplus
}
#endif
#endif

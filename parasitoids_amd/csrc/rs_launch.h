// Launchers of the register-resident kernel families (fft_rs_kernels.h, fft_colfull_kernels.h).
// The 65 sizes x (2 row kernels + 5 full-column kernels) are instantiated in translation units
// of their own (ps_rs_rows.hip, ps_colfull.hip), compiled in parallel with ps_solver.hip; the
// solver sees only these functions.
#pragma once
#include <hip/hip_runtime.h>
#include "fft_kernels.h"

struct ColFullArgs;   // fft_colfull_kernels.h

// per size L = 16 * r2 * r3: row pairs per workgroup of the row kernels, their LDS, whether the
// full-column pass can chain days (state column parked in LDS); false when (r2, r3) is not served
struct RsInfo {
  int np, nthr;
  size_t lds_rows, lds_col1, lds_colc;
  bool chain;
  bool rsp;   // k_row_inv_rsp exists for this size (its staged rows fit in LDS)
};
bool rs_lookup(int L, int* r2, int* r3);
int rs_next_size(int n);   // smallest served size >= n, or 0
bool rs_info(int r2, int r3, RsInfo* out);
int rs_rows_set_attrs();       // hipFuncSetAttribute(MaxDynamicSharedMemorySize) for every row kernel
int rs_colfull_set_attrs();    // ... and every full-column kernel
// launches; return 0 when (r2, r3) is not a served size
int rs_launch_row_fwd(int r2, int r3, const RowFwdArgs& a, int npairs, int batch, hipStream_t st);
int rs_launch_row_inv(int r2, int r3, const RowInvArgs& a, int npairs, int batch, hipStream_t st);
// kernel batches of the full-column pipeline (a.tstride, a.rowrange, a.skip_zero; no pred / trunc_pred):
// persistent workgroups over the live units only (k_row_fwd_rsp); hranges = host copy of a.rowrange.
// An all-empty batch launches nothing.  Sizes with one row pair per workgroup (5600 points among them) keep
// k_row_fwd_rs (rs_fwd_live_ok, ps_rs_rows.hip): the launcher sends them to rs_launch_row_fwd itself.
// rs_row_fwd_info: row pairs per workgroup of the forward row kernels of a size and whether its kernel
// batches go to k_row_fwd_rsp; false when (r2, r3) is not served.
bool rs_row_fwd_info(int r2, int r3, int* np, int* persistent);
// solo: at the sizes with two row pairs per workgroup (5184 and 4608 points among them) launch workgroups of ONE
// pair, two resident per CU, which drift into anti-phase: one transforms while the other's stores are taken.
// stage: the staged kernel (k_row_fwd_rsps: the next unit's source rows copied HBM -> LDS while one is
// transformed) where rs_row_fwd_staged says its LDS fits for rows of a.src_ld doubles; it keeps the workgroup
// of RsCfg::NP pairs and goes before `solo`.
int rs_launch_row_fwd_live(int r2, int r3, const RowFwdArgs& a, const int* hranges, int batch, hipStream_t st,
                           bool stage, bool solo);
// LDS of the staged kernel for source rows of src_ld doubles (0: size not served by the persistent kernels),
// and whether the launcher takes it (<= 160 KB)
size_t rs_row_fwd_stage_lds(int r2, int r3, int src_ld);
bool rs_row_fwd_staged(int r2, int r3, int src_ld);
// live units (np row pairs each) of `nd` entries with source-row ranges [nd][2] under map_wrap(M, P), in
// list order: entry and unit of the first `cap`; returns their number (host only, see ps_row_live_units)
int rs_row_live_units(int P, int M, int np, int nd, const int* ranges, int* day, int* unit, int cap);
// mode 0 (nd >= 1 days), 1, 2, 3 as in fft_colfull_kernels.h; lines8 = 128-byte lines per XCD
int rs_launch_colfull(int r2, int r3, const ColFullArgs& a, int lines8, int batch, hipStream_t st);
// inverse row pass + fold onto the reference torus (PS_MODE_FOLD; k_row_inv_fold), one workgroup per unit
struct RowFoldArgs;
int rs_launch_row_fold(int r2, int r3, const RowFoldArgs& a, int units, hipStream_t st);
// the single-day pass of this size can take the state column from a pending re-transform (ColFullArgs::alt_src)
bool rs_colfull_alt_ok(int r2, int r3);
// two-role chained pass (k_colfull_dual; mode 0, nd >= 2): sizes for which rs_dual_ok
bool rs_dual_ok(int r2, int r3);
// ... and its state-fused instance (ColFullArgs::alt_src set: role A transforms the state column in slot 0
// from the state's row-pass output; one batch entry, no predicate): the sizes that compile it without scratch
bool rs_dual_state_ok(int r2, int r3);
int rs_coldual_set_attrs();
int rs_launch_coldual(int r2, int r3, const ColFullArgs& a, int lines8, int batch, hipStream_t st);

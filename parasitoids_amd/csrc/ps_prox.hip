// Proximity fields (include/parasitoid_hip.h, ps_prox_*): the distance from every cell to the nearest cell of one
// member's own set.  With v the value of input record input[e] -- the one ps_summary_add adds (ps_record_value) -- or
// output input[e] of another fields source, S = {v >= thr[e]} (side 0, "to") or its complement within the domain
// (side 1, "in"),
//   d2_e(y, x) = min { (y - y')^2 + (x - x')^2 : (y', x') in S },  far2 = 2 (N - 1)^2 + 1 where S is empty,
//   Z_e(y, x)  = fl(fl(sqrt((double) d2)) * cell_m).
// Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   Z[e][pitch]          fp64, overwritten by every apply
//   d2[e][pitch]         uint32, likewise
//   g[e][pitch]          uint16: the distance along the own row to the nearest cell of S, 0xffff where the row has none
//   mask[e][pitch / 64]  uint64: S, bit c & 63 of word c >> 6 is cell c (the layout of ps_excur); pad bits 0
// Three launches per apply.  k_prox_mask: one thread per cell, one 64-bit ballot per wave, one lane stores the
// word.  k_prox_rows: one thread per cell counts leading and trailing zeros in its own word and walks the row's
// words outwards (prox_row_dist).  k_prox_cols: a workgroup owns a strip of W columns of one output and a share of
// its rows, stages g of the whole strip in LDS (W * N * 2 B) and every thread searches its column outwards from its
// row until dy^2 >= its best (prox_col_search), then writes d2 and Z.  W is the widest power of two <= 64 whose
// strip fits the LDS one workgroup may hold (64 up to N = 1280 at 160 KiB, 16 at N = 4097, 2 at N = 32767); the
// rows of a strip are shared among as many workgroups as it takes to give every CU one.  One writer per cell, no
// atomics, no hand-off between workgroups, integers until the last two statements: neither W nor the row shares
// change a bit.
#include <math.h>

#include <vector>

#include "ps_common.h"
#include "ps_prox_core.h"

#define PS_PROX_MAX_IN 32      // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_PROX_MAX_OUT 32
#define PX_THREADS 1024        // the column pass: one workgroup per CU (its LDS), 16 waves
#define PX_MAX_SHARES 64       // workgroups that share the rows of one strip

namespace {

struct ProxSlots {
  PsSrc s[PS_PROX_MAX_IN];
};
struct ProxTab {
  int input[PS_PROX_MAX_OUT];
  int side[PS_PROX_MAX_OUT];
  double thr[PS_PROX_MAX_OUT];
};

// blockIdx.y = output; a wave is one mask word
__global__ void __launch_bounds__(256) k_prox_mask(ProxSlots desc, ProxTab tab, uint64_t* __restrict__ mask,
                                                   int64_t ncell, int64_t pitch, double negval) {
  const int e = blockIdx.y;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= pitch) return;   // pitch is a multiple of 64: whole waves leave
  const PsSrc sd = desc.s[tab.input[e]];
  bool in = false;
  if (c < ncell) {
    const double delta = sd.stats ? sd.stats->delta : 0.0;
    const double v = ps_record_value(sd.rec[c], sd.stat_scale, sd.post_scale, delta, negval);
    in = (v >= tab.thr[e]) != (tab.side[e] != 0);
  }
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63) == 0) mask[(int64_t)e * (pitch >> 6) + (c >> 6)] = m;
}

// blockIdx.y = output; one thread per cell
__global__ void __launch_bounds__(256) k_prox_rows(const uint64_t* __restrict__ mask, uint16_t* __restrict__ g, int N,
                                                   int64_t ncell, int64_t pitch) {
  const int e = blockIdx.y;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  const int64_t lo = c / N * N;
  g[(int64_t)e * pitch + c] = (uint16_t)prox_row_dist(mask + (int64_t)e * (pitch >> 6), lo, lo + N - 1, c);
}

// blockIdx.x = strip, blockIdx.y = share of the rows, blockIdx.z = output
__global__ void __launch_bounds__(PX_THREADS) k_prox_cols(const uint16_t* __restrict__ g, uint32_t* __restrict__ d2,
                                                          double* __restrict__ Z, int N, int64_t pitch, int W,
                                                          int rows_per_share, double cell_m) {
  extern __shared__ uint16_t px_lds[];   // [N][W]
  const int e = blockIdx.z;
  const int x0 = blockIdx.x * W;
  const int t = threadIdx.x;
  const int lx = t & (W - 1);
  int ly = t / W;
  if (W == 64) ly = __builtin_amdgcn_readfirstlane(ly);   // the wave, in a scalar register: row tests are uniform
  const int nly = PX_THREADS / W;
  const int x = x0 + lx;
  const uint16_t* __restrict__ ge = g + (int64_t)e * pitch;
  for (int y = ly; y < N; y += nly) px_lds[y * W + lx] = x < N ? ge[(int64_t)y * N + x] : (uint16_t)PROX_NONE;
  __syncthreads();
  if (x >= N) return;
  const uint32_t far2 = prox_far2(N);
  const int y0 = blockIdx.y * rows_per_share;
  const int y1 = min(y0 + rows_per_share, N);
  for (int y = y0 + ly; y < y1; y += nly) {
    const uint32_t best = prox_col_search(px_lds + lx, W, y, N, far2);
    const int64_t c = (int64_t)e * pitch + (int64_t)y * N + x;
    d2[c] = best;
    Z[c] = __dsqrt_rn((double)best) * cell_m;
  }
}

// out[e][k] = Z_e(cell[k]); flat over nout * n
__global__ void k_prox_gather(const double* __restrict__ Z, int64_t pitch, int nout, int64_t n,
                              const int64_t* __restrict__ cell, double* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * nout) return;
  const int64_t e = t / n, k = t - e * n;
  out[t] = Z[e * pitch + cell[k]];
}

}  // namespace

struct ps_prox {
  int device = 0, N = 0, nin = 0, nout = 0;
  int64_t ncell = 0, pitch = 0;
  int wmax = 0, width = 0;         // the widest strip that fits, and the one in use (ps_prox_set_strip)
  int ncu = 0;
  double cell_m = 0.0;
  ProxTab tab;
  double* Z = nullptr;             // [nout][pitch]
  uint32_t* d2 = nullptr;          // [nout][pitch]
  uint16_t* g = nullptr;           // [nout][pitch]
  uint64_t* mask = nullptr;        // [nout][pitch / 64]
  int64_t* g_cell = nullptr;       // gather scratch, grown on demand
  double* g_out = nullptr;
  int64_t g_cap = 0;
  int64_t applies = 0;
  hipStream_t stream = nullptr;    // fetch / gather / apply of another fields source
  PsLastOp last;                   // the last operation on the handle's buffers, on whatever stream it ran
  PsProf prof;                     // channel 0: the mask and the row pass, 1: the column pass
};

extern "C" void ps_prox_destroy(ps_prox* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->last.sync();
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->prof.release();
  for (void* q : {(void*)c->Z, (void*)c->d2, (void*)c->g, (void*)c->mask, (void*)c->g_cell, (void*)c->g_out})
    if (q) (void)hipFree(q);
  c->last.destroy();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int ps_prox_create(int device, int N, int nin, int nout, const int32_t* input, const double* thr,
                              const int32_t* side, double cell_m, ps_prox** out) {
  if (!out || N < 1 || N > PROX_MAX_N || nin < 1 || nin > PS_PROX_MAX_IN || nout < 1 || nout > PS_PROX_MAX_OUT ||
      !input || !thr || !side)
    return ps_fail(PS_ERR_BAD_ARG, "prox_create: N %d (1..%d), %d inputs (1..%d), %d outputs (1..%d)", N, PROX_MAX_N,
                   nin, PS_PROX_MAX_IN, nout, PS_PROX_MAX_OUT);
  if (!(cell_m > 0.0) || !isfinite(cell_m))
    return ps_fail(PS_ERR_BAD_ARG, "prox_create: a cell of %g m", cell_m);
  for (int e = 0; e < nout; ++e) {
    if (input[e] < 0 || input[e] >= nin)
      return ps_fail(PS_ERR_BAD_ARG, "prox_create: output %d reads input %d of %d", e, input[e], nin);
    if (side[e] != 0 && side[e] != 1)
      return ps_fail(PS_ERR_BAD_ARG, "prox_create: side [%d] = %d is neither 0 (to) nor 1 (in)", e, side[e]);
    if (isnan(thr[e])) return ps_fail(PS_ERR_BAD_ARG, "prox_create: thr [%d] is not a number", e);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // Z, d2, g and the mask, checked before anything is allocated
  const size_t z_b = (size_t)nout * pitch * sizeof(double), d_b = (size_t)nout * pitch * sizeof(uint32_t);
  const size_t g_b = (size_t)nout * pitch * sizeof(uint16_t), m_b = (size_t)nout * (pitch >> 6) * sizeof(uint64_t);
  const double need = (double)z_b + (double)d_b + (double)g_b + (double)m_b;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "prox_create: %d outputs x %lld cells x 14.125 B = %.3g GB, %.3g GB free", nout,
                   (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  int lds_max = 0, ncu = 0;
  PS_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  PS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
  if ((int64_t)N * 2 > lds_max)
    return ps_fail(PS_ERR_BAD_ARG, "prox_create: one column of N %d does not fit %d B of LDS", N, lds_max);
  ps_prox* c = new ps_prox();
  c->device = device;
  c->N = N;
  c->nin = nin;
  c->nout = nout;
  c->ncell = ncell;
  c->pitch = pitch;
  c->cell_m = cell_m;
  c->ncu = ncu > 0 ? ncu : 1;
  c->wmax = c->width = prox_strip_width(N, lds_max);
  c->tab = ProxTab();
  for (int e = 0; e < nout; ++e) {
    c->tab.input[e] = input[e];
    c->tab.side[e] = side[e];
    c->tab.thr[e] = thr[e];
  }
  auto fail = [&](int rc) {
    ps_prox_destroy(c);
    return rc;
  };
  // the device's limit, not this handle's need: the attribute is the kernel's, shared by every handle
  hipError_t e = hipFuncSetAttribute((const void*)k_prox_cols, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = c->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&c->Z, z_b);
  if (e == hipSuccess) e = hipMalloc((void**)&c->d2, d_b);
  if (e == hipSuccess) e = hipMalloc((void**)&c->g, g_b);
  if (e == hipSuccess) e = hipMalloc((void**)&c->mask, m_b);
  if (e == hipSuccess) e = hipMemsetAsync(c->Z, 0, z_b, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->d2, 0, d_b, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->g, 0, g_b, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->mask, 0, m_b, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "prox_create: %s", hipGetErrorString(e)));
  *out = c;
  return PS_OK;
}

extern "C" int ps_prox_set_strip(ps_prox* c, int width) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "prox_set_strip: null handle");
  if (width == 0) width = c->wmax;
  if (width < 1 || width > c->wmax || (width & (width - 1)))
    return ps_fail(PS_ERR_BAD_ARG, "prox_set_strip: %d is not a power of two in 1..%d", width, c->wmax);
  c->width = width;
  return PS_OK;
}

// the three launches over the resolved descriptors on `stream`, behind the handle's last operation
static int prox_launch(ps_prox* c, const ProxSlots& desc, hipStream_t stream, double negval) {
  PS_TRY(c->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(c->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_prox_mask, dim3((unsigned)((c->pitch + 255) / 256), c->nout), dim3(256), 0, stream, desc, c->tab,
                     c->mask, c->ncell, c->pitch, negval);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_prox_rows, dim3((unsigned)((c->ncell + 255) / 256), c->nout), dim3(256), 0, stream, c->mask, c->g,
                     c->N, c->ncell, c->pitch);
  PS_HIP(hipGetLastError());
  PS_TRY(c->prof.end(stream, e1));
  PS_TRY(c->prof.begin(1, stream, &e1));
  const int W = c->width;
  const int nstrip = (c->N + W - 1) / W;
  // one workgroup per CU where the strips and outputs alone leave some idle; a share is whole passes of the
  // workgroup's rows
  const int nly = PX_THREADS / W;
  int shares = c->ncu / (nstrip * c->nout);
  shares = shares < 1 ? 1 : shares > PX_MAX_SHARES ? PX_MAX_SHARES : shares;
  int rows = ((c->N + shares - 1) / shares + nly - 1) / nly * nly;
  shares = (c->N + rows - 1) / rows;
  hipLaunchKernelGGL(k_prox_cols, dim3(nstrip, shares, c->nout), dim3(PX_THREADS), (size_t)W * c->N * 2, stream, c->g,
                     c->d2, c->Z, c->N, c->pitch, W, rows, c->cell_m);
  PS_HIP(hipGetLastError());
  PS_TRY(c->prof.end(stream, e1));
  PS_TRY(c->last.mark(stream));
  c->applies += 1;
  return PS_OK;
}

extern "C" int ps_prox_apply(ps_prox* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                             const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                             double negval) {
  if (!c || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "prox_apply: bad arguments");
  if (nin != c->nin) return ps_fail(PS_ERR_BAD_ARG, "prox_apply: %d inputs given, the handle has %d", nin, c->nin);
  PS_HIP(hipSetDevice(c->device));
  // every descriptor first: an apply with a bad record enqueues nothing
  ProxSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("prox_apply", "handle", c->device, c->N, s, nin, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nin; i < PS_PROX_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return prox_launch(c, desc, stream, negval);
}

// the inputs are the current fields of a projection or a release plan (who: the entry point): input i is the
// source's output i, on the handle's stream behind the source's last operation
static int prox_apply_fields(ps_prox* c, void* h, const PsFieldsOps& src, const char* who) {
  if (!c || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  // input i takes Y_i: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  ProxSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "inputs", c->device, c->N, c->nin, h, src, desc.s));
  for (int i = c->nin; i < PS_PROX_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(src.wait(h, c->stream));
  PS_TRY(prox_launch(c, desc, c->stream, 0.0));
  return src.mark(h, c->stream);   // the source's next apply overwrites its fields only after this read
}

extern "C" int ps_prox_apply_project(ps_prox* c, ps_project* p) {
  return prox_apply_fields(c, p, ps_project_fields(), "prox_apply_project");
}

extern "C" int ps_prox_apply_sites(ps_prox* c, ps_sites* p) {
  return prox_apply_fields(c, p, ps_sites_fields(), "prox_apply_sites");
}

// one plane of nbytes per cell to the host, on the handle's stream
static int prox_fetch_plane(ps_prox* c, int e, const void* base, size_t cell_b, void* out, const char* who) {
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (e < 0 || e >= c->nout) return ps_fail(PS_ERR_BAD_ARG, "%s: output %d of %d", who, e, c->nout);
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "%s: nothing applied yet", who);
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(out, (const char*)base + (size_t)e * c->pitch * cell_b, (size_t)c->ncell * cell_b,
                        hipMemcpyDeviceToHost, c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_prox_fetch(ps_prox* c, int e, double* out) {
  return prox_fetch_plane(c, e, c ? c->Z : nullptr, sizeof(double), out, "prox_fetch");
}

extern "C" int ps_prox_fetch_d2(ps_prox* c, int e, uint32_t* out) {
  return prox_fetch_plane(c, e, c ? c->d2 : nullptr, sizeof(uint32_t), out, "prox_fetch_d2");
}

extern "C" int ps_prox_gather(ps_prox* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out) {
  if (!c || n < 0 || (n > 0 && (!rows || !cols || !out))) return ps_fail(PS_ERR_BAD_ARG, "prox_gather: bad arguments");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "prox_gather: nothing applied yet");
  if (n == 0) return PS_OK;
  std::vector<int64_t> cell((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= c->N || cols[k] < 0 || cols[k] >= c->N)
      return ps_fail(PS_ERR_BAD_ARG, "prox_gather: cell %lld = (%d, %d) is outside the %d x %d domain", (long long)k,
                     rows[k], cols[k], c->N, c->N);
    cell[(size_t)k] = (int64_t)rows[k] * c->N + cols[k];
  }
  PS_HIP(hipSetDevice(c->device));
  if (n > c->g_cap) {   // nothing in flight uses the scratch: gather synchronises before it returns
    if (c->g_cell) PS_HIP(hipFree(c->g_cell));
    if (c->g_out) PS_HIP(hipFree(c->g_out));
    c->g_cell = nullptr;
    c->g_out = nullptr;
    c->g_cap = 0;
    PS_HIP(hipMalloc((void**)&c->g_cell, (size_t)n * sizeof(int64_t)));
    PS_HIP(hipMalloc((void**)&c->g_out, (size_t)n * c->nout * sizeof(double)));
    c->g_cap = n;
  }
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(c->g_cell, cell.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  const int64_t total = n * c->nout;
  hipLaunchKernelGGL(k_prox_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->Z, c->pitch,
                     c->nout, n, c->g_cell, c->g_out);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, c->g_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_prox_info(ps_prox* c, int* N, int* nin, int* nout, int64_t* applies, int* strip) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "prox_info: null handle");
  if (N) *N = c->N;
  if (nin) *nin = c->nin;
  if (nout) *nout = c->nout;
  if (applies) *applies = c->applies;
  if (strip) *strip = c->width;
  return PS_OK;
}

extern "C" int ps_prox_prof(ps_prox* c, int enable, double* row_ms, int64_t* row_n, double* col_ms, int64_t* col_n) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "prox_prof: null handle");
  PS_HIP(hipSetDevice(c->device));
  c->prof.set(enable);
  if (row_ms || row_n) PS_TRY(c->prof.totals(0, row_ms, row_n));
  if (col_ms || col_n) PS_TRY(c->prof.totals(1, col_ms, col_n));
  return PS_OK;
}

static int prox_view(void* h, PsProjectView* out) {
  ps_prox* c = static_cast<ps_prox*>(h);
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "prox view: null handle");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "nothing applied yet: apply the proximity fields first");
  out->Y = c->Z;
  out->pitch = c->pitch;
  out->N = c->N;
  out->nout = c->nout;
  out->device = c->device;
  return PS_OK;
}
static int prox_wait(void* h, hipStream_t stream) { return static_cast<ps_prox*>(h)->last.wait(stream); }
static int prox_mark(void* h, hipStream_t stream) { return static_cast<ps_prox*>(h)->last.mark(stream); }
PsFieldsOps ps_prox_fields() { return PsFieldsOps{"proximity fields", prox_view, prox_wait, prox_mark}; }

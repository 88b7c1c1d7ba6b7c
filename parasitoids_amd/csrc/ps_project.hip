// Projections over time (include/parasitoid_hip.h, ps_project_*): linear functionals of one member's daily
// fields, Y_e(c) = sum_d W[e][d] v_d(c), computed on the device from the solver's records.  The value v_d of
// a record is the one ps_summary_add adds (ps_record_value).  Layout (pitch = N*N rounded up to 64 cells, as
// ps_summary.hip):
//   Y[e][pitch]        fp64, overwritten by every apply, zeros included
//   tiles[ntile]       per tile of PS_PROJ_TILE outputs the input records with a non-zero weight in the tile,
//                      in ascending d, and their weights [entry][output of the tile]; built and uploaded at create
// One thread owns a pair of cells and keeps one tile of outputs in registers; blockIdx.y runs over the
// tiles, so a record is read once per tile that uses it and never for a tile that does not.  The sum starts
// from +0.0, walks the records in ascending d and rounds the product and the sum separately, so a host loop
// acc = acc + W[e, d] * v_d reproduces it bit for bit (a zero weight adds +0.0 or -0.0 to acc >= +0.0: no
// bit changes, so the entries of a tile's list need no test per output).  Every cell has one writer: no
// atomics, the same call gives the same bits.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_PROJ_MAX_IN 32    // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_PROJ_MAX_OUT 32
#define PS_PROJ_TILE 8       // outputs per thread: 2 cells x 8 fp64 accumulators = 32 VGPRs
#define PS_PROJ_THREADS 256

namespace {

struct ProjSlots {
  PsSrc s[PS_PROJ_MAX_IN];
};
struct ProjTile {
  double w[PS_PROJ_MAX_IN][PS_PROJ_TILE];   // [entry][output of the tile]; 0 past nout
  int rec[PS_PROJ_MAX_IN];                  // the input record of every entry, ascending
  int n, pad_;
};

__device__ inline void proj_load(const double* __restrict__ rec, bool pair, int64_t i, double2& r) {
  if (pair)
    r = *reinterpret_cast<const double2*>(rec + i);
  else
    r = make_double2(rec[i], 0.0);
}

// blockIdx.y = output tile; thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd N*N
// alone).  The tile's list and weights are the same for every lane (scalar loads); the record of entry
// q + 1 is loaded while entry q is accumulated.
__global__ void __launch_bounds__(PS_PROJ_THREADS) k_project_apply(ProjSlots desc, const ProjTile* __restrict__ tiles,
                                                                   double* __restrict__ Y, int nout, int64_t ncell,
                                                                   int64_t pitch, double negval) {
  __shared__ double sdelta[PS_PROJ_MAX_IN];
  const ProjTile* __restrict__ tl = tiles + blockIdx.y;
  const int n = tl->n;
  for (int q = threadIdx.x; q < n; q += blockDim.x) {
    const ps_day_stats* st = desc.s[tl->rec[q]].stats;
    sdelta[q] = st ? st->delta : 0.0;
  }
  __syncthreads();
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  if (!(pair || tail)) return;
  const int64_t i = pair ? 2 * j : ncell - 1;
  double a0[PS_PROJ_TILE], a1[PS_PROJ_TILE];
#pragma unroll
  for (int t = 0; t < PS_PROJ_TILE; ++t) a0[t] = a1[t] = 0.0;
  int d = __builtin_amdgcn_readfirstlane(tl->rec[0]);   // n >= 1: no output row is all zeros
  double2 r;
  proj_load(desc.s[d].rec, pair, i, r);
  for (int q = 0; q < n; ++q) {
    double2 rn = make_double2(0.0, 0.0);
    int dn = d;
    if (q + 1 < n) {
      dn = __builtin_amdgcn_readfirstlane(tl->rec[q + 1]);
      proj_load(desc.s[dn].rec, pair, i, rn);
    }
    const double ss = desc.s[d].stat_scale, ps = desc.s[d].post_scale;
    const double delta = sdelta[q];
    const double v0 = ps_record_value(r.x, ss, ps, delta, negval);
    const double v1 = pair ? ps_record_value(r.y, ss, ps, delta, negval) : 0.0;
#pragma unroll
    for (int t = 0; t < PS_PROJ_TILE; ++t) {
      const double w = tl->w[q][t];
      a0[t] = __dadd_rn(a0[t], __dmul_rn(w, v0));
      a1[t] = __dadd_rn(a1[t], __dmul_rn(w, v1));
    }
    r = rn;
    d = dn;
  }
  const int e0 = blockIdx.y * PS_PROJ_TILE;
#pragma unroll
  for (int t = 0; t < PS_PROJ_TILE; ++t) {
    if (e0 + t < nout) {
      double* y = Y + (int64_t)(e0 + t) * pitch + i;
      if (pair)
        *reinterpret_cast<double2*>(y) = make_double2(a0[t], a1[t]);
      else
        *y = a0[t];
    }
  }
}

// out[e][k] = Y_e(cell[k]); flat over nout * n
__global__ void k_project_gather(const double* __restrict__ Y, int64_t pitch, int nout, int64_t n,
                                 const int64_t* __restrict__ cell, double* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * nout) return;
  const int64_t e = t / n, k = t - e * n;
  out[t] = Y[e * pitch + cell[k]];
}

}  // namespace

struct ps_project {
  int device = 0, N = 0, nin = 0, nout = 0, ntile = 0;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                    // blocks of one apply launch per tile
  std::vector<ProjTile> host_tiles;
  ProjTile* tiles = nullptr;       // [ntile]
  double* Y = nullptr;             // [nout][pitch]
  int64_t* g_cell = nullptr;       // gather scratch, grown on demand
  double* g_out = nullptr;
  int64_t g_cap = 0;
  int64_t applies = 0;
  hipStream_t stream = nullptr;    // fetch / gather
  PsLastOp last;                   // the last operation on Y, on whatever stream it ran
  PsProf prof;                     // channel 0: the applies
};

extern "C" void ps_project_destroy(ps_project* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  p->last.sync();
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  p->prof.release();
  for (void* q : {(void*)p->tiles, (void*)p->Y, (void*)p->g_cell, (void*)p->g_out})
    if (q) (void)hipFree(q);
  p->last.destroy();
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

extern "C" int ps_project_create(int device, int N, int nin, int nout, const double* W, ps_project** out) {
  if (!out || N < 1 || nin < 1 || nin > PS_PROJ_MAX_IN || nout < 1 || nout > PS_PROJ_MAX_OUT || !W)
    return ps_fail(PS_ERR_BAD_ARG, "project_create: N %d, %d inputs (1..%d), %d outputs (1..%d)", N, nin,
                   PS_PROJ_MAX_IN, nout, PS_PROJ_MAX_OUT);
  for (int e = 0; e < nout; ++e) {
    bool any = false;
    for (int d = 0; d < nin; ++d) {
      const double w = W[(size_t)e * nin + d];
      if (!isfinite(w) || w < 0.0)
        return ps_fail(PS_ERR_BAD_ARG, "project_create: weight [%d][%d] = %g is not finite and >= 0", e, d, w);
      any = any || w != 0.0;
    }
    if (!any) return ps_fail(PS_ERR_BAD_ARG, "project_create: output %d has no non-zero weight", e);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_PROJ_THREADS - 1) / PS_PROJ_THREADS;   // the pairs and the tail thread
  if (nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "project_create: N %d is too large for one launch", N);
  const int ntile = (nout + PS_PROJ_TILE - 1) / PS_PROJ_TILE;
  // everything, checked before anything is allocated: the output fields and the tile tables
  const double need = (double)nout * pitch * 8.0 + (double)ntile * sizeof(ProjTile);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "project_create: %d outputs x %lld cells x 8 B = %.3g GB, %.3g GB free", nout,
                   (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_project* p = new ps_project();
  p->device = device;
  p->N = N;
  p->nin = nin;
  p->nout = nout;
  p->ntile = ntile;
  p->ncell = ncell;
  p->pitch = pitch;
  p->nblk = (int)nblk;
  p->host_tiles.resize((size_t)ntile);
  for (int T = 0; T < ntile; ++T) {
    ProjTile& tl = p->host_tiles[(size_t)T];
    tl = ProjTile();
    for (int d = 0; d < nin; ++d) {
      bool used = false;
      for (int t = 0; t < PS_PROJ_TILE; ++t) {
        const int e = T * PS_PROJ_TILE + t;
        used = used || (e < nout && W[(size_t)e * nin + d] != 0.0);
      }
      if (!used) continue;
      for (int t = 0; t < PS_PROJ_TILE; ++t) {
        const int e = T * PS_PROJ_TILE + t;
        tl.w[tl.n][t] = e < nout ? W[(size_t)e * nin + d] : 0.0;
      }
      tl.rec[tl.n++] = d;
    }
  }
  auto fail = [&](int rc) {
    ps_project_destroy(p);
    return rc;
  };
  const size_t tile_b = (size_t)ntile * sizeof(ProjTile), y_b = (size_t)nout * pitch * sizeof(double);
  hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = p->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&p->tiles, tile_b);
  if (e == hipSuccess) e = hipMalloc((void**)&p->Y, y_b);
  if (e == hipSuccess) e = hipMemcpyAsync(p->tiles, p->host_tiles.data(), tile_b, hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(p->Y, 0, y_b, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "project_create: %s", hipGetErrorString(e)));
  *out = p;
  return PS_OK;
}

extern "C" int ps_project_apply(ps_project* p, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                                const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                                double negval) {
  if (!p || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "project_apply: bad arguments");
  if (nin != p->nin) return ps_fail(PS_ERR_BAD_ARG, "project_apply: %d inputs given, the handle has %d", nin, p->nin);
  PS_HIP(hipSetDevice(p->device));
  // every descriptor first: an apply with a bad record enqueues nothing
  ProjSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("project_apply", "handle", p->device, p->N, s, nin, kind, idx, stat_scale, post_scale,
                         use_delta, false, desc.s, &stream));
  for (int i = nin; i < PS_PROJ_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_TRY(p->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(p->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_project_apply, dim3(p->nblk, p->ntile), dim3(PS_PROJ_THREADS), 0, stream, desc, p->tiles, p->Y,
                     p->nout, p->ncell, p->pitch, negval);
  PS_HIP(hipGetLastError());
  PS_TRY(p->prof.end(stream, e1));
  PS_TRY(p->last.mark(stream));
  p->applies += 1;
  return PS_OK;
}

extern "C" int ps_project_fetch(ps_project* p, int e, double* out) {
  if (!p || !out) return ps_fail(PS_ERR_BAD_ARG, "project_fetch: bad arguments");
  if (e < 0 || e >= p->nout) return ps_fail(PS_ERR_BAD_ARG, "project_fetch: output %d of %d", e, p->nout);
  if (p->applies == 0) return ps_fail(PS_ERR_STATE, "project_fetch: nothing projected yet");
  PS_HIP(hipSetDevice(p->device));
  PS_TRY(p->last.wait(p->stream));
  PS_HIP(hipMemcpyAsync(out, p->Y + (int64_t)e * p->pitch, (size_t)p->ncell * sizeof(double), hipMemcpyDeviceToHost,
                        p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  return PS_OK;
}

extern "C" int ps_project_gather(ps_project* p, int64_t n, const int32_t* rows, const int32_t* cols, double* out) {
  if (!p || n < 0 || (n > 0 && (!rows || !cols || !out))) return ps_fail(PS_ERR_BAD_ARG, "project_gather: bad arguments");
  if (p->applies == 0) return ps_fail(PS_ERR_STATE, "project_gather: nothing projected yet");
  if (n == 0) return PS_OK;
  std::vector<int64_t> cell((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= p->N || cols[k] < 0 || cols[k] >= p->N)
      return ps_fail(PS_ERR_BAD_ARG, "project_gather: cell %lld = (%d, %d) is outside the %d x %d domain", (long long)k,
                     rows[k], cols[k], p->N, p->N);
    cell[(size_t)k] = (int64_t)rows[k] * p->N + cols[k];
  }
  PS_HIP(hipSetDevice(p->device));
  if (n > p->g_cap) {   // the handle's stream is idle here: fetch and gather synchronise before they return
    if (p->g_cell) PS_HIP(hipFree(p->g_cell));
    if (p->g_out) PS_HIP(hipFree(p->g_out));
    p->g_cell = nullptr;
    p->g_out = nullptr;
    p->g_cap = 0;
    PS_HIP(hipMalloc((void**)&p->g_cell, (size_t)n * sizeof(int64_t)));
    PS_HIP(hipMalloc((void**)&p->g_out, (size_t)n * p->nout * sizeof(double)));
    p->g_cap = n;
  }
  PS_TRY(p->last.wait(p->stream));
  PS_HIP(hipMemcpyAsync(p->g_cell, cell.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, p->stream));
  const int64_t total = n * p->nout;
  hipLaunchKernelGGL(k_project_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, p->stream, p->Y, p->pitch,
                     p->nout, n, p->g_cell, p->g_out);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, p->g_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  return PS_OK;
}

extern "C" int ps_project_info(ps_project* p, int* N, int* nin, int* nout, int64_t* applies) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "project_info: null handle");
  if (N) *N = p->N;
  if (nin) *nin = p->nin;
  if (nout) *nout = p->nout;
  if (applies) *applies = p->applies;
  return PS_OK;
}

extern "C" int ps_project_prof(ps_project* p, int enable, double* total_ms, int64_t* launches) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "project_prof: null handle");
  PS_HIP(hipSetDevice(p->device));
  p->prof.set(enable);
  if (total_ms || launches) PS_TRY(p->prof.totals(0, total_ms, launches));
  return PS_OK;
}

static int proj_view(void* h, PsProjectView* out) {
  ps_project* p = static_cast<ps_project*>(h);
  if (!p || !out) return ps_fail(PS_ERR_BAD_ARG, "project view: null handle");
  if (p->applies == 0) return ps_fail(PS_ERR_STATE, "nothing projected yet: apply the projection first");
  out->Y = p->Y;
  out->pitch = p->pitch;
  out->N = p->N;
  out->nout = p->nout;
  out->device = p->device;
  return PS_OK;
}
static int proj_wait(void* h, hipStream_t stream) { return static_cast<ps_project*>(h)->last.wait(stream); }
static int proj_mark(void* h, hipStream_t stream) { return static_cast<ps_project*>(h)->last.mark(stream); }
PsFieldsOps ps_project_fields() { return PsFieldsOps{"projection", proj_view, proj_wait, proj_mark}; }

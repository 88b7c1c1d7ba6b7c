// Neighbourhood fields (include/parasitoid_hip.h, ps_nbhd_*): the largest value of one member's field within a
// disc, Z_e(y, x) = max { v(y', x') : 0 <= y', x' < N, (y' - y)^2 + (x' - x)^2 <= r2[e] }, v the value of input
// record input[e] -- the one ps_summary_add adds (ps_record_value) -- or output input[e] of another fields source.
// Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   Z[e][pitch]          fp64, overwritten by every apply, zeros included
//   flag[nin][ntile]     int32, rewritten by every apply with the skip on: does tile t of input i hold a value != 0
// The disc is a stack of horizontal chords of half-width w(dy) = floor(sqrt(r2 - dy^2)), so
//   Z(y, x) = max_dy rowmax_{w(dy)}(y + dy, x),   rowmax_w(y, x) = max v(y, [x - w, x + w] clipped to the domain),
// and a row maximum over len cells starting at a is max(L_k(a), L_k(a + len - 2^k)), k = floor(log2 len), with
// L_k(y, x) = max v(y, x .. x + 2^k - 1).  One workgroup owns a tile of NB_TY x NB_TX outputs of one pass (an input
// and up to NB_CHUNK of the outputs that read it, grouped by input as CatchTab groups them): it stages v of the tile
// and a halo of H cells -- the cells of the domain only; what lies outside is neither loaded nor read -- into LDS,
// and then walks the levels k = 0, 1, ..: every thread folds the chords whose clipped length has floor(log2) == k
// into register accumulators that start from the centre cell, then the workgroup doubles the windows in place,
// L_{k+1}(x) = max(L_k(x), L_k(x + 2^k)) (read into registers, barrier, write, barrier).  Work per output cell is
// two LDS reads per chord, 2 (2H + 1) in all, and 3 LDS accesses per staged cell and level: it grows like H, not
// like the H^2 cells of the disc.  A maximum is exact, so neither the tile nor the order changes a bit.  One writer
// per cell, no atomics, no hand-off between workgroups.  With the skip on, a pre-pass writes per input and tile
// whether the tile holds a value != 0 (one writer per flag); a tile whose own and eight neighbouring tiles are all
// empty -- they cover its haloed window, H <= NB_TY -- stores zeros without staging: the maximum of zeros.
#include <math.h>

#include <utility>
#include <vector>

#include "ps_common.h"

#define PS_NBHD_MAX_IN 32      // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_NBHD_MAX_OUT 32
#define NB_TY 32               // the tile of outputs; the halo must not exceed either edge (the 3 x 3 flags)
#define NB_TX 64
#define NB_THREADS 512         // 8 waves: wave j owns the tile rows j, j + 8, j + 16, j + 24
#define NB_CELLS (NB_TY * NB_TX / NB_THREADS)
#define NB_CHUNK 8             // outputs of one pass: NB_CHUNK x NB_CELLS fp64 accumulators per thread
#define NB_WAVES (NB_THREADS / 64)
#define NB_LEVELS 7            // floor(log2(2 * 32 + 1)) + 1
// the haloed tile at the largest halo, per thread: wave j owns its rows j, j + 8, .., a lane the columns l, l + 64
#define NB_SROWS ((NB_TY + 2 * PS_NBHD_MAX_HALF + NB_WAVES - 1) / NB_WAVES)
#define NB_SCOLS ((NB_TX + 2 * PS_NBHD_MAX_HALF + 63) / 64)

static_assert(PS_NBHD_MAX_HALF <= NB_TY && PS_NBHD_MAX_HALF <= NB_TX, "the 3 x 3 tile flags must cover the halo");
static_assert(NB_TX == 64 && NB_TY % NB_WAVES == 0, "one wave per tile row");

namespace {

struct NbhdSlots {
  PsSrc s[PS_NBHD_MAX_IN];
};
// the outputs in group order (ascending input, the outputs of one input in ascending e, as CatchTab); pass p reads
// input pin[p] and owns the entries pstart[p] .. pstart[p + 1] - 1, at most NB_CHUNK of them
struct NbhdTab {
  int out[PS_NBHD_MAX_OUT];       // the output an entry writes
  int half[PS_NBHD_MAX_OUT];      // H = floor(sqrt(r2)) of the entry
  int pin[PS_NBHD_MAX_OUT];
  int phalf[PS_NBHD_MAX_OUT];     // the largest H of the pass: its halo
  int pstart[PS_NBHD_MAX_OUT + 1];
  int npass, pad_;
  unsigned char w[PS_NBHD_MAX_OUT][PS_NBHD_MAX_HALF + 1];   // chord half-width at |dy| = 0 .. H
  // the chords |dy| <= dmax[q][k] have a full length 2 w + 1 of level floor(log2) >= k (w falls with |dy|); -1: none
  signed char dmax[PS_NBHD_MAX_OUT][NB_LEVELS + 1];
};

// flag[i][t] = does tile t of input i hold a value != 0; one workgroup per (tile, input), thread 0 writes
__global__ void __launch_bounds__(256) k_nbhd_flags(NbhdSlots desc, int* __restrict__ flag, int N, int ntx, int nty,
                                                    double negval) {
  const int tx = blockIdx.x, ty = blockIdx.y, d = blockIdx.z;
  const double* __restrict__ rec = desc.s[d].rec;
  const ps_day_stats* st = desc.s[d].stats;
  const double ss = desc.s[d].stat_scale, ps = desc.s[d].post_scale;
  const double delta = st ? st->delta : 0.0;
  const int x = tx * NB_TX + (threadIdx.x & (NB_TX - 1));
  int any = 0;
  if (x < N)
    for (int r = threadIdx.x / NB_TX; r < NB_TY; r += 256 / NB_TX) {
      const int y = ty * NB_TY + r;
      if (y >= N) break;
      any |= ps_record_value(rec[(int64_t)y * N + x], ss, ps, delta, negval) != 0.0;
    }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flag[((int64_t)d * nty + ty) * ntx + tx] = any;
}

// floor(log2(len)), len >= 1
__device__ inline int nb_level(int len) { return 31 - __clz(len); }

__global__ void __launch_bounds__(NB_THREADS) k_nbhd_apply(NbhdSlots desc, NbhdTab tab, double* __restrict__ Z,
                                                           const int* __restrict__ flag, int N, int64_t pitch,
                                                           int ntx, int nty, double negval) {
  extern __shared__ double nb_lds[];   // [rows of the haloed tile][NB_TX + 2 hp]
  const int tx = blockIdx.x, ty = blockIdx.y, p = blockIdx.z;
  const int d = tab.pin[p], hp = tab.phalf[p];
  const int q0 = tab.pstart[p], nq = tab.pstart[p + 1] - q0;
  const int x0 = tx * NB_TX, y0 = ty * NB_TY;
  const int t = threadIdx.x;
  const int lx = t & (NB_TX - 1);
  const int ly = __builtin_amdgcn_readfirstlane(t / NB_TX);   // the wave, in a scalar register: row tests are uniform
  const int x = x0 + lx;

  if (flag) {   // the own and the eight neighbouring tiles cover the haloed window
    int any = 0;
    for (int j = max(ty - 1, 0); j <= min(ty + 1, nty - 1); ++j)
      for (int i = max(tx - 1, 0); i <= min(tx + 1, ntx - 1); ++i) any |= flag[((int64_t)d * nty + j) * ntx + i];
    if (!any) {
      if (x < N)
        for (int c = 0; c < nq; ++c)
          for (int i = 0; i < NB_CELLS; ++i) {
            const int y = y0 + ly + i * NB_WAVES;
            if (y < N) Z[(int64_t)tab.out[q0 + c] * pitch + (int64_t)y * N + x] = 0.0;
          }
      return;
    }
  }

  // the haloed window, clipped to the domain: global rows gy0 .. gy1 and columns gx0 .. gx1; LDS cell (r, c) is
  // the global cell (y0 - hp + r, x0 - hp + c)
  const int oy = y0 - hp, ox = x0 - hp;
  const int ldw = NB_TX + 2 * hp;
  const int gy0 = max(oy, 0), gy1 = min(y0 + NB_TY - 1 + hp, N - 1);
  const int gx0 = max(ox, 0), gx1 = min(x0 + NB_TX - 1 + hp, N - 1);
  const int nrow = gy1 - gy0 + 1, ncol = gx1 - gx0 + 1;
  {
    const double* __restrict__ rec = desc.s[d].rec;
    const ps_day_stats* st = desc.s[d].stats;
    const double ss = desc.s[d].stat_scale, ps = desc.s[d].post_scale;
    const double delta = st ? st->delta : 0.0;
    // every load of the thread is issued before the first value is used: one memory latency per tile, not one per cell
    double sv[NB_SROWS][NB_SCOLS];
#pragma unroll
    for (int u = 0; u < NB_SROWS; ++u)
#pragma unroll
      for (int s = 0; s < NB_SCOLS; ++s) {
        const int r = ly + u * NB_WAVES, c = lx + s * 64;
        if (r < nrow && c < ncol) sv[u][s] = rec[(int64_t)(gy0 + r) * N + gx0 + c];
      }
#pragma unroll
    for (int u = 0; u < NB_SROWS; ++u)
#pragma unroll
      for (int s = 0; s < NB_SCOLS; ++s) {
        const int r = ly + u * NB_WAVES, c = lx + s * 64;
        if (r < nrow && c < ncol)
          nb_lds[(gy0 + r - oy) * ldw + (gx0 + c - ox)] = ps_record_value(sv[u][s], ss, ps, delta, negval);
      }
  }
  __syncthreads();

  // the accumulators start from the centre cell: no sentinel
  double acc[NB_CHUNK][NB_CELLS];
  bool live[NB_CELLS];
  int ctr[NB_CELLS];   // the centre cell in LDS: inside the allocation also where the cell lies outside the domain
#pragma unroll
  for (int i = 0; i < NB_CELLS; ++i) {
    const int y = y0 + ly + i * NB_WAVES;
    live[i] = x < N && y < N;
    ctr[i] = (y - oy) * ldw + (x - ox);
    const double v = live[i] ? nb_lds[ctr[i]] : 0.0;
#pragma unroll
    for (int c = 0; c < NB_CHUNK; ++c) acc[c][i] = v;
  }

  // lane l holds the chord half-width at |dy| = l of every output of the pass: read back by lane index below
  int wreg[NB_CHUNK];
#pragma unroll
  for (int c = 0; c < NB_CHUNK; ++c) wreg[c] = (c < nq && lx <= PS_NBHD_MAX_HALF) ? tab.w[q0 + c][lx] : 0;

  // no column of the tile's chords is clipped: the level of a chord is that of its full length, for every thread,
  // and level k visits the chords of level k alone; in a clipped tile clipping only shortens a chord, so it visits
  // those of a full level >= k and every lane tests its own clipped length
  const bool xin = ox >= 0 && x0 + NB_TX - 1 + hp <= N - 1;
  const int kmax = nb_level(2 * hp + 1);
  for (int k = 0; k <= kmax; ++k) {
    const int span = 1 << k;
#pragma unroll
    for (int c = 0; c < NB_CHUNK; ++c) {
      if (c >= nq) break;
      const int q = q0 + c;
      const int dk = tab.dmax[q][k];
      const int d0 = xin ? tab.dmax[q][k + 1] + 1 : 0;
      for (int ady = d0; ady <= dk; ++ady) {
        const int w = __builtin_amdgcn_readlane(wreg[c], ady);
        const int a = max(x - w, 0), b = min(x + w, N - 1);
        const bool mine = nb_level(b - a + 1) == k;
        // the rows -ady and +ady (the centre row twice: a maximum does not mind) of the thread's cells, every read
        // issued before the first is used; a chord that is not this lane's, or whose row lies outside the domain,
        // reads the cell's own centre instead and is dropped
#pragma unroll
        for (int sg = -1; sg <= 1; sg += 2)
#pragma unroll
          for (int i = 0; i < NB_CELLS; ++i) {
            const int yy = y0 + ly + i * NB_WAVES + sg * ady;
            const bool ok = live[i] && mine && yy >= 0 && yy < N;
            const int row = (yy - oy) * ldw - ox;
            const double v = fmax(nb_lds[ok ? row + a : ctr[i]], nb_lds[ok ? row + b - span + 1 : ctr[i]]);
            acc[c][i] = ok ? fmax(acc[c][i], v) : acc[c][i];
          }
      }
    }
    if (k == kmax) break;
    // L_{k+1}(x) = max(L_k(x), L_k(x + 2^k)) wherever the doubled window stays inside the staged columns
    const int nc = ncol - 2 * span + 1;
    double m[NB_SROWS][NB_SCOLS];
#pragma unroll
    for (int u = 0; u < NB_SROWS; ++u)
#pragma unroll
      for (int s = 0; s < NB_SCOLS; ++s) {
        const int r = ly + u * NB_WAVES, c = lx + s * 64;
        if (r < nrow && c < nc) {
          const double* cell = nb_lds + (gy0 + r - oy) * ldw + (gx0 + c - ox);
          m[u][s] = fmax(cell[0], cell[span]);
        }
      }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NB_SROWS; ++u)
#pragma unroll
      for (int s = 0; s < NB_SCOLS; ++s) {
        const int r = ly + u * NB_WAVES, c = lx + s * 64;
        if (r < nrow && c < nc) nb_lds[(gy0 + r - oy) * ldw + (gx0 + c - ox)] = m[u][s];
      }
    __syncthreads();
  }

#pragma unroll
  for (int c = 0; c < NB_CHUNK; ++c) {
    if (c >= nq) break;
    double* z = Z + (int64_t)tab.out[q0 + c] * pitch;
#pragma unroll
    for (int i = 0; i < NB_CELLS; ++i) {
      const int y = y0 + ly + i * NB_WAVES;
      if (live[i]) z[(int64_t)y * N + x] = acc[c][i];
    }
  }
}

// out[e][k] = Z_e(cell[k]); flat over nout * n
__global__ void k_nbhd_gather(const double* __restrict__ Z, int64_t pitch, int nout, int64_t n,
                              const int64_t* __restrict__ cell, double* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * nout) return;
  const int64_t e = t / n, k = t - e * n;
  out[t] = Z[e * pitch + cell[k]];
}

}  // namespace

struct ps_nbhd {
  int device = 0, N = 0, nin = 0, nout = 0;
  int64_t ncell = 0, pitch = 0;
  int ntx = 0, nty = 0;            // tiles of one field
  int hmax = 0;                    // the largest halo of the handle
  size_t lds = 0;                  // dynamic LDS of one apply workgroup
  bool skip = true;                // the empty-tile pre-pass
  NbhdTab tab;
  double* Z = nullptr;             // [nout][pitch]
  int* flag = nullptr;             // [nin][nty][ntx]
  int64_t* g_cell = nullptr;       // gather scratch, grown on demand
  double* g_out = nullptr;
  int64_t g_cap = 0;
  int64_t applies = 0;
  hipStream_t stream = nullptr;    // fetch / gather / apply of another fields source
  PsLastOp last;                   // the last operation on Z, on whatever stream it ran
  PsProf prof;                     // channel 0: the applies
};

extern "C" void ps_nbhd_destroy(ps_nbhd* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->last.sync();
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->prof.release();
  for (void* q : {(void*)c->Z, (void*)c->flag, (void*)c->g_cell, (void*)c->g_out})
    if (q) (void)hipFree(q);
  c->last.destroy();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// floor(sqrt(v)) of a small whole number
static int nbhd_isqrt(int64_t v) {
  int64_t r = (int64_t)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return (int)r;
}

extern "C" int ps_nbhd_create(int device, int N, int nin, int nout, const int32_t* input, const int32_t* r2,
                              ps_nbhd** out) {
  if (!out || N < 1 || nin < 1 || nin > PS_NBHD_MAX_IN || nout < 1 || nout > PS_NBHD_MAX_OUT || !input || !r2)
    return ps_fail(PS_ERR_BAD_ARG, "nbhd_create: N %d, %d inputs (1..%d), %d outputs (1..%d)", N, nin,
                   PS_NBHD_MAX_IN, nout, PS_NBHD_MAX_OUT);
  const int r2max = (PS_NBHD_MAX_HALF + 1) * (PS_NBHD_MAX_HALF + 1) - 1;
  for (int e = 0; e < nout; ++e) {
    if (input[e] < 0 || input[e] >= nin)
      return ps_fail(PS_ERR_BAD_ARG, "nbhd_create: output %d reads input %d of %d", e, input[e], nin);
    if (r2[e] < 0 || r2[e] > r2max)
      return ps_fail(PS_ERR_BAD_ARG, "nbhd_create: r2 [%d] = %d is not in 0..%d (a half-width of at most %d cells)", e,
                     r2[e], r2max, PS_NBHD_MAX_HALF);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int ntx = (N + NB_TX - 1) / NB_TX, nty = (N + NB_TY - 1) / NB_TY;
  if (nty > 65535) return ps_fail(PS_ERR_BAD_ARG, "nbhd_create: N %d is too large for one launch", N);
  // the output fields and the tile flags, checked before anything is allocated
  const size_t flag_b = (size_t)nin * ntx * nty * sizeof(int);
  const double need = (double)nout * pitch * 8.0 + (double)flag_b;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "nbhd_create: %d outputs x %lld cells x 8 B = %.3g GB, %.3g GB free", nout,
                   (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_nbhd* c = new ps_nbhd();
  c->device = device;
  c->N = N;
  c->nin = nin;
  c->nout = nout;
  c->ncell = ncell;
  c->pitch = pitch;
  c->ntx = ntx;
  c->nty = nty;
  NbhdTab& tab = c->tab;
  tab = NbhdTab();
  int q = 0;
  for (int d = 0; d < nin; ++d) {   // ascending input, the outputs of one input in ascending e; chunks of NB_CHUNK
    for (int e = 0; e < nout; ++e) {
      if (input[e] != d) continue;
      const int h = nbhd_isqrt(r2[e]);
      if (tab.npass == 0 || tab.pin[tab.npass - 1] != d || q - tab.pstart[tab.npass - 1] == NB_CHUNK) {
        tab.pin[tab.npass] = d;
        tab.phalf[tab.npass] = 0;
        tab.pstart[tab.npass++] = q;
      }
      tab.out[q] = e;
      tab.half[q] = h;
      for (int dy = 0; dy <= h; ++dy) tab.w[q][dy] = (unsigned char)nbhd_isqrt((int64_t)r2[e] - (int64_t)dy * dy);
      for (int k = 0; k <= NB_LEVELS; ++k) {
        int d = -1;
        while (d < h && (2 * tab.w[q][d + 1] + 1) >> k) ++d;   // 2 w + 1 >= 2^k
        tab.dmax[q][k] = (signed char)d;
      }
      if (h > tab.phalf[tab.npass - 1]) tab.phalf[tab.npass - 1] = h;
      if (h > c->hmax) c->hmax = h;
      tab.pstart[tab.npass] = ++q;
    }
  }
  c->lds = (size_t)(NB_TY + 2 * c->hmax) * (NB_TX + 2 * c->hmax) * sizeof(double);
  auto fail = [&](int rc) {
    ps_nbhd_destroy(c);
    return rc;
  };
  const size_t z_b = (size_t)nout * pitch * sizeof(double);
  hipError_t e = hipFuncSetAttribute((const void*)k_nbhd_apply, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (NB_TY + 2 * PS_NBHD_MAX_HALF) * (NB_TX + 2 * PS_NBHD_MAX_HALF) * 8);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = c->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&c->Z, z_b);
  if (e == hipSuccess) e = hipMalloc((void**)&c->flag, flag_b);
  if (e == hipSuccess) e = hipMemsetAsync(c->Z, 0, z_b, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->flag, 0, flag_b, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "nbhd_create: %s", hipGetErrorString(e)));
  *out = c;
  return PS_OK;
}

extern "C" int ps_nbhd_set_skip(ps_nbhd* c, int on) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "nbhd_set_skip: null handle");
  c->skip = on != 0;
  return PS_OK;
}

// the pre-pass and the apply over the resolved descriptors on `stream`, behind the handle's last operation
static int nbhd_launch(ps_nbhd* c, const NbhdSlots& desc, hipStream_t stream, double negval) {
  PS_TRY(c->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(c->prof.begin(0, stream, &e1));
  if (c->skip) {
    hipLaunchKernelGGL(k_nbhd_flags, dim3(c->ntx, c->nty, c->nin), dim3(256), 0, stream, desc, c->flag, c->N, c->ntx,
                       c->nty, negval);
    PS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_nbhd_apply, dim3(c->ntx, c->nty, c->tab.npass), dim3(NB_THREADS), c->lds, stream, desc, c->tab,
                     c->Z, c->skip ? c->flag : nullptr, c->N, c->pitch, c->ntx, c->nty, negval);
  PS_HIP(hipGetLastError());
  PS_TRY(c->prof.end(stream, e1));
  PS_TRY(c->last.mark(stream));
  c->applies += 1;
  return PS_OK;
}

extern "C" int ps_nbhd_apply(ps_nbhd* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                             const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                             double negval) {
  if (!c || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "nbhd_apply: bad arguments");
  if (nin != c->nin) return ps_fail(PS_ERR_BAD_ARG, "nbhd_apply: %d inputs given, the handle has %d", nin, c->nin);
  PS_HIP(hipSetDevice(c->device));
  // every descriptor first: an apply with a bad record enqueues nothing
  NbhdSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("nbhd_apply", "handle", c->device, c->N, s, nin, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nin; i < PS_NBHD_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return nbhd_launch(c, desc, stream, negval);
}

// the inputs are the current fields of a projection or a release plan (who: the entry point): input i is the
// source's output i, on the handle's stream behind the source's last operation
static int nbhd_apply_fields(ps_nbhd* c, void* h, const PsFieldsOps& src, const char* who) {
  if (!c || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  // input i takes Y_i: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  NbhdSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "inputs", c->device, c->N, c->nin, h, src, desc.s));
  for (int i = c->nin; i < PS_NBHD_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(src.wait(h, c->stream));
  PS_TRY(nbhd_launch(c, desc, c->stream, 0.0));
  return src.mark(h, c->stream);   // the source's next apply overwrites its fields only after this read
}

extern "C" int ps_nbhd_apply_project(ps_nbhd* c, ps_project* p) {
  return nbhd_apply_fields(c, p, ps_project_fields(), "nbhd_apply_project");
}

extern "C" int ps_nbhd_apply_sites(ps_nbhd* c, ps_sites* p) {
  return nbhd_apply_fields(c, p, ps_sites_fields(), "nbhd_apply_sites");
}

extern "C" int ps_nbhd_fetch(ps_nbhd* c, int e, double* out) {
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "nbhd_fetch: bad arguments");
  if (e < 0 || e >= c->nout) return ps_fail(PS_ERR_BAD_ARG, "nbhd_fetch: output %d of %d", e, c->nout);
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "nbhd_fetch: nothing applied yet");
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(out, c->Z + (int64_t)e * c->pitch, (size_t)c->ncell * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_nbhd_gather(ps_nbhd* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out) {
  if (!c || n < 0 || (n > 0 && (!rows || !cols || !out))) return ps_fail(PS_ERR_BAD_ARG, "nbhd_gather: bad arguments");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "nbhd_gather: nothing applied yet");
  if (n == 0) return PS_OK;
  std::vector<int64_t> cell((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= c->N || cols[k] < 0 || cols[k] >= c->N)
      return ps_fail(PS_ERR_BAD_ARG, "nbhd_gather: cell %lld = (%d, %d) is outside the %d x %d domain", (long long)k,
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
  hipLaunchKernelGGL(k_nbhd_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->Z, c->pitch,
                     c->nout, n, c->g_cell, c->g_out);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, c->g_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_nbhd_info(ps_nbhd* c, int* N, int* nin, int* nout, int64_t* applies) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "nbhd_info: null handle");
  if (N) *N = c->N;
  if (nin) *nin = c->nin;
  if (nout) *nout = c->nout;
  if (applies) *applies = c->applies;
  return PS_OK;
}

extern "C" int ps_nbhd_prof(ps_nbhd* c, int enable, double* total_ms, int64_t* launches) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "nbhd_prof: null handle");
  PS_HIP(hipSetDevice(c->device));
  c->prof.set(enable);
  if (total_ms || launches) PS_TRY(c->prof.totals(0, total_ms, launches));
  return PS_OK;
}

static int nbhd_view(void* h, PsProjectView* out) {
  ps_nbhd* c = static_cast<ps_nbhd*>(h);
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "nbhd view: null handle");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "nothing applied yet: apply the neighbourhood fields first");
  out->Y = c->Z;
  out->pitch = c->pitch;
  out->N = c->N;
  out->nout = c->nout;
  out->device = c->device;
  return PS_OK;
}
static int nbhd_wait(void* h, hipStream_t stream) { return static_cast<ps_nbhd*>(h)->last.wait(stream); }
static int nbhd_mark(void* h, hipStream_t stream) { return static_cast<ps_nbhd*>(h)->last.mark(stream); }
PsFieldsOps ps_nbhd_fields() { return PsFieldsOps{"neighbourhood fields", nbhd_view, nbhd_wait, nbhd_mark}; }

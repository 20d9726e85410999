// Max-value entropy search (Wang & Jegelka, ICML 2017), the expensive half: quantiles of the distribution of the grid's own
// MINIMUM value y* under one hyper sample's posterior (the library minimises), found on the device without random numbers.
// No counterpart in the reference's scores/.
//
// Rows of a sample (mu_j, var_j), j < M:
//   bad    mu or var NaN, or var < 0     score NaN (score.hip)          take no part in anything below
//   exact  var == 0                      score exactly 0.0              take no part in anything below
//   live   the rest, sigma_j = sqrt(var_j)
// With independent candidates the grid minimum survives y with log-probability
//   L(y) = sum_{live j} log Phi((mu_j - y)/sigma_j)                     non-increasing in y
// and y*_k, k = 1..K, is the root of L(y) = t_k = log1p(-u_k), u_k = (k - 1/2)/K.
//   bracket   lo0 = min_j (mu_j - 10 sigma_j),  hi0 = min_j (mu_j + 10 sigma_j)       operation order: s = sqrt(var); t = s * 10;
//             lo = mu - t; hi = mu + t; minima over the live rows -- every step one rounded operation, a minimum rounds nothing,
//             so lo0 / hi0 are the same bits whatever the decomposition.  L(hi0) <= log Phi(-10) ~ -53 < t_k; L(lo0) ~ -7.6e-24 M > t_k.
//   round     P = 15 interior probes y_p = lo + (hi - lo) * (p/16), p = 1..P (p/16 exact); n = #{p : L(y_p) > t_k};
//             [lo, hi] <- [y_n, y_n+1] with y_0 = lo, y_P+1 = hi.  R = 10 rounds: 16^10 >= 1e12.
//   result    y*_k = (lo + hi) / 2 of the last bracket.
// No live row: lo0 = hi0 = NaN and every y*_k is NaN (no live row is there to read it).
//
// Launches: one fused min-reduction for lo0 / hi0, then one per round covering all S x K x P probes: R + 1 in all, no host round
// trip.  grid.y = sample, grid.x = nb = the row blocks (a function of M alone), so a sample meets the same decomposition whether
// it is searched alone or beside the others: the per-sample loop and the one-call nomination get the same bits.  Within a
// round's block a 16-lane group shares one row and its lanes take the probes (the 16th lane idles): one copy of the log Phi code,
// one running sum per thread -- fifteen sums per thread, unrolled, would be fifteen inlined copies of erfc / erfcx / log / log1p.
// Per-thread sums in row order, lanes 16 and 32 apart by shuffles, the four waves in order, one partial per (block, k, p); the
// LAST block of a sample to arrive (a ticket from one atomic counter per sample, the pattern of score.hip's
// block_best_ticket_record) adds the partials in block order and narrows that sample's K brackets in place.  No atomics on
// doubles, nothing depends on arrival order: bit-reproducible call to call.
#pragma clang fp contract(off)
#include "b7_internal.h"
#include "mes_math.h"

namespace {

constexpr int MES_P = 15;   // interior probes per round; P + 1 = 16 lanes per row
constexpr int MES_R = 10;   // rounds: (P + 1)^R = 2^40 >= 1e12
constexpr int MES_ROWS = 16;  // rows a 256-thread block takes per pass

// c->ystar as the kernels address it, for mes_S samples, mes_K levels and mes_nb row blocks (mes_begin)
struct MesBuf {
  double *ystar;    // [S][K]
  double *b0;       // [S][2] lo0, hi0
  double *br;       // [S][K][2] the brackets
  double *minpart;  // [S][nb][3] the first launch's partials: lo, hi, "no live row" (1.0 / 0.0)
  double *part;     // [S][nb][K][P] a round's partial sums
  unsigned *ticket; // [S]
};
MesBuf mes_buf(const b7_ctx *c) {
  const size_t S = (size_t)c->mes_S, K = (size_t)c->mes_K, nb = (size_t)c->mes_nb;
  MesBuf b;
  b.ystar = (double *)c->ystar.p;
  b.b0 = b.ystar + S * K;
  b.br = b.b0 + S * 2;
  b.minpart = b.br + S * K * 2;
  b.part = b.minpart + S * nb * 3;
  b.ticket = (unsigned *)c->mes_ticket.p;
  return b;
}
size_t mes_doubles(size_t S, size_t K, size_t nb) { return S * K + S * 2 + S * K * 2 + S * nb * 3 + S * nb * K * MES_P; }

__device__ __forceinline__ bool live_row(double m, double v) { return v > 0.0 && m == m; }
__device__ __forceinline__ double min2(double a, double b) { return (b < a) ? b : a; }

// every thread calls; true in every thread of the block that drew the sample's last ticket (n_arrivals of them), whose loads
// from here on see what the other blocks stored before their tickets.  flag: one LDS word
__device__ __forceinline__ bool last_arrival(unsigned *__restrict__ ticket, unsigned n_arrivals, unsigned *flag) {
  __threadfence();  // this thread's partials are visible device-wide before the ticket is taken
  __syncthreads();
  if (threadIdx.x == 0) *flag = (atomicAdd(ticket, 1u) == n_arrivals - 1) ? 1u : 0u;
  __syncthreads();
  if (!*flag) return false;
  __threadfence();
  return true;
}
__device__ __forceinline__ double agent_load(const double *p) {  // another CU's partial, not a stale line of this CU's cache
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lo0 / hi0 of sample blockIdx.y (slot slot0 + blockIdx.y), and its K brackets set to them
__global__ void __launch_bounds__(256)
    mes_bracket_kernel(const double *__restrict__ mu, const double *__restrict__ var, long long stride, long long M, int slot0, int K,
                       MesBuf b) {
  __shared__ double sh[4][3];
  __shared__ unsigned flag;
  const int s = blockIdx.y, slot = slot0 + s, nb = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *m = mu + (long long)s * stride, *v = var + (long long)s * stride;
  double r[3] = {INFINITY, INFINITY, 1.0};
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < M; j += (long long)nb * 256) {
    const double mj = m[j], vj = v[j];
    if (live_row(mj, vj)) {
      const double t = sqrt(vj) * 10.0;
      r[0] = min2(r[0], mj - t);
      r[1] = min2(r[1], mj + t);
      r[2] = 0.0;
    }
  }
  double *mine = b.minpart + ((size_t)s * nb + blockIdx.x) * 3;
  for (int pass = 0; pass < 2; ++pass) {  // 0: this block's rows -> its partial; 1 (the last block only): the partials -> the result
    for (int e = 0; e < 3; ++e) {
      for (int o = 32; o > 0; o >>= 1) r[e] = min2(r[e], __shfl_xor(r[e], o));
      if (lane == 0) sh[wave][e] = r[e];
    }
    __syncthreads();
    for (int e = 0; e < 3; ++e) r[e] = min2(min2(sh[0][e], sh[1][e]), min2(sh[2][e], sh[3][e]));
    __syncthreads();
    if (pass == 1) break;
    if (threadIdx.x == 0) mine[0] = r[0], mine[1] = r[1], mine[2] = r[2];
    if (!last_arrival(b.ticket + slot, (unsigned)nb, &flag)) return;
    r[0] = INFINITY, r[1] = INFINITY, r[2] = 1.0;
    for (int q = threadIdx.x; q < nb; q += 256)
      for (int e = 0; e < 3; ++e) r[e] = min2(r[e], agent_load(b.minpart + ((size_t)s * nb + q) * 3 + e));
  }
  const double lo0 = (r[2] == 0.0) ? r[0] : NAN, hi0 = (r[2] == 0.0) ? r[1] : NAN;
  if (threadIdx.x == 0) {
    b.b0[slot * 2] = lo0, b.b0[slot * 2 + 1] = hi0;
    b.ticket[slot] = 0u;  // ready for the next launch (stream order: nobody else touches it meanwhile)
  }
  for (int k = threadIdx.x; k < K; k += 256) b.br[((size_t)slot * K + k) * 2] = lo0, b.br[((size_t)slot * K + k) * 2 + 1] = hi0;
}

// one round: the P probes of level k = blockIdx.z of sample blockIdx.y over this block's rows; the sample's last block narrows
__global__ void __launch_bounds__(256)
    mes_round_kernel(const double *__restrict__ mu, const double *__restrict__ var, long long stride, long long M, int slot0, int K,
                     MesBuf b) {
  __shared__ double sh[4][16];
  __shared__ double Ls[B7_MES_KMAX * MES_P];
  __shared__ unsigned flag;
  const int s = blockIdx.y, k = blockIdx.z, slot = slot0 + s, nb = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = threadIdx.x & 15, rsub = threadIdx.x >> 4;  // probe p + 1 (p == 15 idles) of row rsub of each pass
  const double *m = mu + (long long)s * stride, *v = var + (long long)s * stride;
  const double *bk = b.br + ((size_t)slot * K + k) * 2;
  const double lo = bk[0], hi = bk[1];
  const double y = lo + ((hi - lo) * ((double)(p + 1) * 0.0625));
  double acc = 0.0;
  if (p < MES_P)
    for (long long base = (long long)blockIdx.x * 256; base < M; base += (long long)nb * 256)
      for (int i = 0; i < 256 / MES_ROWS; ++i) {
        const long long j = base + i * MES_ROWS + rsub;
        if (j < M) {
          const double mj = m[j], vj = v[j];
          if (live_row(mj, vj)) acc = acc + b7_log_ndtr((mj - y) / sqrt(vj));
        }
      }
  acc = acc + __shfl_xor(acc, 16);
  acc = acc + __shfl_xor(acc, 32);
  if (lane < 16) sh[wave][lane] = acc;
  __syncthreads();
  const size_t KP = (size_t)K * MES_P;
  if (threadIdx.x < MES_P)
    b.part[((size_t)s * nb + blockIdx.x) * KP + (size_t)k * MES_P + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
  if (!last_arrival(b.ticket + slot, (unsigned)nb * (unsigned)K, &flag)) return;
  // L at every probe of every level of this sample: the partials in block order
  for (int q = threadIdx.x; q < (int)KP; q += 256) {
    double a = 0.0;
    for (int blk = 0; blk < nb; ++blk) a = a + agent_load(b.part + ((size_t)s * nb + blk) * KP + q);
    Ls[q] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) b.ticket[slot] = 0u;
  for (int kk = threadIdx.x; kk < K; kk += 256) {
    double *bq = b.br + ((size_t)slot * K + kk) * 2;
    const double l0 = bq[0], h0 = bq[1], w = h0 - l0;
    const double t = log1p(-(((double)(kk + 1) - 0.5) / (double)K));
    int n = 0;
    for (int q = 0; q < MES_P; ++q) n += (Ls[kk * MES_P + q] > t) ? 1 : 0;
    const double l1 = (n == 0) ? l0 : l0 + (w * ((double)n * 0.0625));
    const double h1 = (n == MES_P) ? h0 : l0 + (w * ((double)(n + 1) * 0.0625));
    bq[0] = l1, bq[1] = h1;
    b.ystar[(size_t)slot * K + kk] = (l1 + h1) * 0.5;
  }
}

int mes_blocks(const b7_ctx *c, int64_t M) {  // score.hip's nblocks: a function of M (and the device) alone
  const int64_t nb = (M + 255) / 256, cap = (int64_t)c->cus * 8;
  return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

}  // namespace

// c->ystar laid out for S samples of M rows at K levels, the tickets zeroed; what the buffer held is gone
int mes_begin(b7_ctx *c, int S, int64_t M, int K) {
  if (S < 1 || M < 1 || K < 1 || K > B7_MES_KMAX) return b7_fail(c, B7_ERR_INVALID, "mes: S >= 1, M >= 1 and 1 <= K <= %d", B7_MES_KMAX);
  const int nb = mes_blocks(c, M);
  B7_TRY(b7_ensure(c, c->ystar, sizeof(double) * mes_doubles((size_t)S, (size_t)K, (size_t)nb)));
  B7_TRY(b7_ensure(c, c->mes_ticket, sizeof(unsigned) * (size_t)S));
  B7_HIP(c, hipMemsetAsync(c->mes_ticket.p, 0, sizeof(unsigned) * (size_t)S, c->stream));
  c->mes_S = S, c->mes_K = K, c->mes_nb = nb, c->mes_M = M, c->mes_valid = false;
  return B7_OK;
}

// y* of nS samples (sample s at mu / var + s * stride, M = c->mes_M rows each) into slots [slot0, slot0 + nS) of the layout
// mes_begin made: R + 1 launches on the stream
int launch_mes_search(b7_ctx *c, const double *mu, const double *var, int64_t stride, int nS, int slot0) {
  if (nS < 1 || slot0 < 0 || slot0 + nS > c->mes_S) return b7_fail(c, B7_ERR_STATE, "mes: samples [%d, %d) outside the %d laid out", slot0, slot0 + nS, c->mes_S);
  const MesBuf b = mes_buf(c);
  const long long M = (long long)c->mes_M;
  const int K = c->mes_K, nb = c->mes_nb;
  {
    PhaseScope ps(c, "mes");
    hipLaunchKernelGGL(mes_bracket_kernel, dim3(nb, nS), dim3(256), 0, c->stream, mu, var, (long long)stride, M, slot0, K, b);
  }
  for (int r = 0; r < MES_R; ++r) {
    PhaseScope ps(c, "mes");
    hipLaunchKernelGGL(mes_round_kernel, dim3(nb, nS, K), dim3(256), 0, c->stream, mu, var, (long long)stride, M, slot0, K, b);
  }
  B7_HIP(c, hipGetLastError());
  c->mes_valid = true;
  return B7_OK;
}

// where sample `slot`'s K values of y* are (device), for ScoreParams
const double *mes_ystar_dev(const b7_ctx *c, int slot) { return (const double *)c->ystar.p + (size_t)slot * c->mes_K; }

static int mes_upload(b7_ctx *c, const double *mean, const double *var, int64_t M) {
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (size_t)M));
  B7_TRY(b7_ensure(c, c->tmpvar, sizeof(double) * (size_t)M));
  B7_HIP(c, hipMemcpyAsync(c->tmpmu.p, mean, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(c->tmpvar.p, var, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  return B7_OK;
}

extern "C" {

int b7_mes_set_levels(b7_ctx *c, int K) {
  if (!c) return B7_ERR_INVALID;
  if (K < 1 || K > B7_MES_KMAX) return b7_fail(c, B7_ERR_INVALID, "mes_set_levels: K = %d outside 1..%d", K, B7_MES_KMAX);
  c->mes_levels = K;
  return B7_OK;
}

int b7_mes_last_ystar(b7_ctx *c, int *S, int *K, double *ystar, double *bracket) {
  if (!c) return B7_ERR_INVALID;
  if (!c->mes_valid) return b7_fail(c, B7_ERR_STATE, "mes_last_ystar: no y* search has run on this context");
  B7_HIP(c, hipSetDevice(c->device));
  if (S) *S = c->mes_S;
  if (K) *K = c->mes_K;
  const MesBuf b = mes_buf(c);
  if (ystar) B7_HIP(c, hipMemcpyAsync(ystar, b.ystar, sizeof(double) * (size_t)c->mes_S * c->mes_K, hipMemcpyDeviceToHost, c->stream));
  if (bracket) B7_HIP(c, hipMemcpyAsync(bracket, b.b0, sizeof(double) * (size_t)c->mes_S * 2, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_mes_ystar(b7_ctx *c, const double *mean, const double *var, int64_t M, int K, double *ystar, double *bracket) {
  if (!c) return B7_ERR_INVALID;
  if (K < 1 || K > B7_MES_KMAX) return b7_fail(c, B7_ERR_INVALID, "mes_ystar: K = %d outside 1..%d", K, B7_MES_KMAX);
  if (M < 1 || !mean || !var || !ystar) return b7_fail(c, B7_ERR_INVALID, "mes_ystar: bad arguments");
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(mes_upload(c, mean, var, M));
  B7_TRY(mes_begin(c, 1, M, K));
  B7_TRY(launch_mes_search(c, (const double *)c->tmpmu.p, (const double *)c->tmpvar.p, 0, 1, 0));
  return b7_mes_last_ystar(c, nullptr, nullptr, ystar, bracket);
}

int b7_mes_compute(b7_ctx *c, const double *mean, const double *var, const double *ystar, int K, int64_t M, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (K < 1 || K > B7_MES_KMAX) return b7_fail(c, B7_ERR_INVALID, "mes_compute: K = %d outside 1..%d", K, B7_MES_KMAX);
  if (M < 0 || !ystar || (M > 0 && (!mean || !var || !out))) return b7_fail(c, B7_ERR_INVALID, "mes_compute: bad arguments");
  if (M == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(mes_upload(c, mean, var, M));
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)M));
  // the caller's y* goes to a buffer of its own: the last search's y* (b7_mes_last_ystar) stays what it was
  B7_TRY(b7_ensure(c, c->mes_user, sizeof(double) * B7_MES_KMAX));
  B7_HIP(c, hipMemcpyAsync(c->mes_user.p, ystar, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, c->stream));
  ScoreParams p;
  p.kind = B7_SCORE_MES, p.ystar = (const double *)c->mes_user.p, p.nlev = K;
  B7_TRY(launch_score(c, p, (const double *)c->tmpmu.p, (const double *)c->tmpvar.p, M, 1, (double *)c->tmpgrid.p, false));
  B7_HIP(c, hipMemcpyAsync(out, c->tmpgrid.p, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

}  // extern "C"

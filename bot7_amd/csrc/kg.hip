// The knowledge gradient: a one-step look-ahead nomination -- b7_kg_nominate, b7_kg_last, b7_kg_compute.
//
// No counterpart in the reference.  Frazier, Powell & Dayanik (INFORMS J. Comput. 2009); Scott, Frazier & Powell (SIAM J. Optim.
// 2011) for Gaussian processes.  The library minimises: under hyper sample s, with a discretisation set A of n <= 16 grid rows a_i,
//   KG_s(x) = min_i alpha_i - E_Z[min_i (alpha_i + b_i Z)],      Z ~ N(0, 1),
//   alpha_i = mu_s(a_i),  b_i = c_i(x) / sqrt(t(x)),  c_i(x) = k_s(x, a_i) - K*_s(x, X) W_s[:, i],  W_s[:, i] = inv(K_s) k_s(X, a_i),
//   t(x) = var_s(x) + noise_s (+ the jitter of a redo); line 0 is the candidate's own, alpha_0 = mu_s(x), b_0 = var_s(x) / sqrt(t(x)),
//   left out when x is itself a row of A (by row index).
// Per call: eval_enqueue's fits and posteriors with a BelKeep (mu, var [S][M]); the rows of A (the caller's, or the n lowest of the
// marginal mean, chosen on the device); per sample the scaled points of A and alpha; the columns k_s(X, a_i) (kg_kernel's column
// pass over the observations); W by the two triangular mat-vecs that make alpha (launch_alpha_batch, once per point); kg_kernel
// over the grid; the fold over the samples into the accumulator; the existing score:div / arg-max / record.  One host wait.
//
// kg_kernel is believer_kernel (batch.hip) with sixteen columns in w_j's place: the same slabs of 64 observations (32 for dpad >=
// 48) double-buffered in LDS, the same argument (c - xs/2) - zs/2, the same epilogue function cov_nonpos4<KERN>, K* never stored.
// It keeps a text of its own beside the slab walk of ksx_walk.h: written on the walk, its 32-row classes (dpad >= 48) came out with
// one LDS read more per slab than this text (a paired read of W's rows split in two); only the dpad / covariance switch is shared.
// OPERAND ORDER, fixed whatever the grid's size: the distance product takes the OBSERVATIONS as its A operand and the queries as
// its B operand, so that a 16 x 16 tile of K* comes out as D[obs = lq + 4 r][query = lr] -- which is, register r by register r,
// the A operand (row = query lr, k = lq) of the next product over the observations 16 t + 4 r + {0, 1, 2, 3}: four MFMAs per tile
// against W's rows from LDS, no LDS round trip for K*.  The sum over the observations runs slabs, tiles and r in ascending order.
// The product's accumulator is D[query = lq + 4 r][line = lr]: a lane holds one line of four queries, a query's sixteen lines sit
// in one 16-lane row.  k(x, a_i) is one more tile (queries as A, the points of A as B, scaled as prep_obs_kernel scales an
// observation) in that same layout.  The epilogue stays in those registers: kg_envelope below.
//
// The expectation in Frazier's positive-term form, sum over the lines of the lower envelope with a finite right breakpoint z_i of
// (b_i - b_next(i)) f(-|z_i|), f(z) = phi(z) + z Phi(z): no sort and no data-dependent loop.  Line i lives on [lo_i, hi_i],
//   hi_i = min_{j: b_j < b_i} (alpha_j - alpha_i) / (b_i - b_j)   (next(i): the j that attains it; among equal quotients the smaller slope),
//   lo_i = max_{j: b_j > b_i} (alpha_i - alpha_j) / (b_j - b_i),
// equal slopes keep the smaller intercept, then the lower index (the own line is index 0), and i is on the envelope iff lo_i < hi_i.
// Phi and phi through ocml's erfc and exp, contraction off.  Padding lines (index > n) take no part, by index.
#include <string.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"
#include "gemm_f64.h"
#include "ksx_exp.h"
#include "ksx_walk.h"

namespace {

constexpr int KQ = 64;                 // query rows per block (16 per wave), as believer_kernel's BQ
constexpr int KL = B7_KG_MAX_POINTS;   // lines beside the own one = columns of W = lanes of a row
constexpr int WST = KL + 1;            // row stride of a slab of W in LDS
__host__ __device__ constexpr int kg_slab(int dpad) { return dpad >= 48 ? 32 : 64; }

// ---- the envelope --------------------------------------------------------------------------------------------------------
// f(z) = phi(z) + z Phi(z) for z <= 0
__device__ __forceinline__ double kg_f(double z) {
#pragma clang fp contract(off)
  const double pdf = exp((z * z) * -0.5) * 0.39894228040143267794;   // 1/sqrt(2 pi)
  const double cdf = erfc(z * -0.70710678118654752440) * 0.5;        // erfc(-z/sqrt2)/2
  const double f = pdf + z * cdf;
  return f > 0.0 ? f : 0.0;
}

struct KgSeg {
  double lo, hi, bn;  // the line's interval, and the slope of the line that takes over at hi
  bool dead;          // no part: padding, or an equal slope with a smaller intercept (then a lower index) exists
};

// line (a, b) meets line (aj, bj) (on: that line takes part; j_first: it has the lower index)
__device__ __forceinline__ void kg_meet(double a, double b, double aj, double bj, bool on, bool j_first, KgSeg &g) {
#pragma clang fp contract(off)
  const bool below = on && bj < b, above = on && bj > b;
  const double num = below ? aj - a : a - aj;
  const double den = below ? b - bj : bj - b;
  const double z = num / den;
  if (below && (z < g.hi || (z == g.hi && bj < g.bn))) g.hi = z, g.bn = bj;
  if (above && z > g.lo) g.lo = z;
  if (on && bj == b && (aj < a || (aj == a && j_first))) g.dead = true;
}

__device__ __forceinline__ double kg_term(double b, const KgSeg &g) {
#pragma clang fp contract(off)
  const bool in = !g.dead && g.lo < g.hi && g.hi < INFINITY;
  const double t = (b - g.bn) * kg_f(in ? -fabs(g.hi) : 0.0);
  return in ? t : 0.0;
}

// One query per 16-lane row: lane lr holds line 1 + lr = (a, b), taking part for lr < n; (a0, b0) is line 0, the query's own
// (own: it takes part).  Returns the expectation's decrease, the same value on every lane of the row.  Every lane of the wave
// must call it.  The row sum is the xor tree 1, 2, 4, 8, the own line's term added last.
__device__ __forceinline__ double kg_envelope(double a, double b, int n, double a0, double b0, bool own, int lane) {
  const int lr = lane & 15, row = lane & 48;
  const bool live = lr < n;
  KgSeg g{-INFINITY, INFINITY, 0.0, !live};
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    const double aj = __shfl(a, row | j), bj = __shfl(b, row | j);
    kg_meet(a, b, aj, bj, j != lr, j < lr, g);
  }
  kg_meet(a, b, a0, b0, own, true, g);
  // the own line against this lane's, then over the row: lo by max, (hi, bn) by the lexicographic min, dead by or
  KgSeg g0{-INFINITY, INFINITY, 0.0, !own};
  kg_meet(a0, b0, a, b, live, false, g0);
  int dead0 = g0.dead ? 1 : 0;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const double lo = __shfl_xor(g0.lo, o), hi = __shfl_xor(g0.hi, o), bn = __shfl_xor(g0.bn, o);
    dead0 |= __shfl_xor(dead0, o);
    if (lo > g0.lo) g0.lo = lo;
    if (hi < g0.hi || (hi == g0.hi && bn < g0.bn)) g0.hi = hi, g0.bn = bn;
  }
  g0.dead = dead0 != 0;
  double t = kg_term(b, g);
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o);
  return t + kg_term(b0, g0);
}

// ---- the pass over the grid (or, column != 0, over the observations) ---------------------------------------------------------
struct KgPass {
  const double *xq; int64_t rows;       // candidate rows (or the N raw observations)
  const double *w, *zsc, *zss;          // the S fits (strides dpad, Npad dpad, Npad)
  const double *W;                      // [KL][S][Npad] inv(K_s) k_s(X, a_i); only i < n is read
  const double *par;                    // [S][2] amp, noise + jitter
  const double *sa, *ha, *al;           // [S][KL][dpad] the points of A scaled, [S][KL] their zs/2, [S][KL] mu_s(a_i)
  const long long *arows;               // [KL] the rows of A (0-based)
  const double *mu, *var;               // [S][M]
  double *kcol;                         // column pass: [KL][S][Npad] out
  double *v;                            // [S][M] out
  double *slopes;                       // [S][M][n + 1] out, or null
  int n;
};

template <int DPAD, int KERN>
__global__ void __launch_bounds__(256) kg_kernel(KgPass p, int d, int Npad, int N, int column) {
  extern __shared__ __align__(16) double sm[];
  const int64_t s = blockIdx.z, S = gridDim.z;
  const double *w = p.w + s * DPAD, *zsc = p.zsc + s * (int64_t)Npad * DPAD, *zsh = p.zss + s * Npad;
  const double amp = p.par[2 * s], tnoise = p.par[2 * s + 1];
  const int64_t Mtotal = p.rows;
  const int n = p.n;
  constexpr int KO = kg_slab(DPAD);
  constexpr int TPR = 256 / KO;
  constexpr int dpad = DPAD, NCH = (DPAD / 2 + TPR - 1) / TPR, KSTEPS = DPAD / 4, NW = KO * KL / 256;
  constexpr int stride = DPAD + 1;
  constexpr int R0 = (KQ * stride > 2 * KO * stride) ? KQ * stride : 2 * KO * stride;
  double *sq = sm;                          // KQ x stride, prologue only
  double *so = sm;                          // 2 x KO x stride, from the first slab on
  double *sh = sm + R0;                     // 2 x KO        zs/2 of the slab
  double *sw = sh + 2 * KO;                 // 2 x KO x WST  W's rows of the slab
  double *shq = sw + 2 * KO * WST;          // KQ            xs/2 of the queries
  double *stab = shq + KQ;                  // 128           amp * 2^(j/128)
  double *sxa = stab + 128;                 // KL x stride   the points of A, scaled
  double *sha = sxa + KL * stride;          // KL            their zs/2 (1e300 in the padding -> exactly 0)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t qbase = (int64_t)blockIdx.x * KQ;
  const int srow = tid / TPR, sq4 = tid % TPR;
  const int qrow = tid >> 2, qq4 = tid & 3;
  constexpr int half = DPAD >> 1;

  if (tid < 128) stab[tid] = amp * b7_exp2_tab_dev[tid];
  {
    int64_t g = qbase + qrow;
    if (g > Mtotal - 1) g = Mtotal - 1;
    for (int k = qq4; k < dpad; k += 4) sq[qrow * stride + k] = (k < d) ? p.xq[g * d + k] : 0.0;
  }
  for (int e = tid; e < KL * dpad; e += 256) sxa[(e / dpad) * stride + (e % dpad)] = p.sa[s * KL * dpad + e];
  if (tid >= 128 && tid < 128 + KL) sha[tid - 128] = p.ha[s * KL + (tid - 128)];
  const int nslab = column ? 0 : Npad / KO;

  d2_t pre[NCH];
  double pre_h = 0.0, pre_w[NW];
  auto load_slab = [&](int sl) {
    const double *src = zsc + (int64_t)(sl * KO + srow) * dpad;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int kc = i * TPR + sq4;
      if (kc < half) pre[i] = *reinterpret_cast<const d2_t *>(src + 2 * kc);
    }
    if (tid < KO) pre_h = zsh[sl * KO + tid];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int e = tid + 256 * i, col = e / KO, row = e % KO;
      pre_w[i] = (col < n) ? p.W[((int64_t)col * S + s) * Npad + sl * KO + row] : 0.0;
    }
  };
  auto store_slab = [&](int buf) {
    double *dst = so + buf * KO * stride + srow * stride;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int kc = i * TPR + sq4;
      if (kc < half) {
        dst[2 * kc] = pre[i][0];
        dst[2 * kc + 1] = pre[i][1];
      }
    }
    if (tid < KO) sh[buf * KO + tid] = pre_h;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int e = tid + 256 * i, col = e / KO, row = e % KO;
      sw[buf * KO * WST + row * WST + col] = pre_w[i];
    }
  };

  if (nslab > 0) load_slab(0);
  __syncthreads();  // query tile visible
  if (tid < KQ) {
    double a = 0.0;
    for (int k = 0; k < dpad; ++k) {
      double x = sq[tid * stride + k];
      a += (x * x) * w[k];
    }
    shq[tid] = 0.5 * a;
  }
  double qf[KSTEPS];  // this lane's query fragments: query row (wave*16 + lr), k = 4 k4 + lq -- an A or a B operand alike
#pragma unroll
  for (int k4 = 0; k4 < KSTEPS; ++k4) qf[k4] = sq[(wave * 16 + lr) * stride + lq + 4 * k4];
  __syncthreads();  // every wave holds its fragments, shq is complete: the region now belongs to the slabs
  if (nslab > 0) store_slab(0);
  __syncthreads();

  const double hql = shq[wave * 16 + lr];  // xs/2 of the query this lane's K* entries belong to
  d4_t wacc = {0.0, 0.0, 0.0, 0.0};        // sum_obs K*(query lq + 4 r, obs) W(obs, line lr)

  int cur = 0;
  for (int sl = 0; sl < nslab; ++sl) {
    const bool more = (sl + 1) < nslab;
    if (more) load_slab(sl + 1);
    const double *sob = so + cur * KO * stride;
    const double *swb = sw + cur * KO * WST;
#pragma unroll
    for (int t = 0; t < KO / 16; ++t) {
      const double *ob = sob + (t * 16 + lr) * stride + lq;
      d4_t c = {0.0, 0.0, 0.0, 0.0};
      {
        double bf[KSTEPS];
#pragma unroll
        for (int k4 = 0; k4 < KSTEPS; ++k4) bf[k4] = ob[4 * k4];
#pragma unroll
        for (int k4 = 0; k4 < KSTEPS; ++k4) c = mfma_f64(bf[k4], qf[k4], c);  // D[obs lq + 4 r][query lr]
      }
      double kv[4], arg[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) arg[r] = (c[r] - hql) - sh[cur * KO + t * 16 + lq + 4 * r];
      cov_nonpos4<KERN>(arg, stab, kv);
#pragma unroll
      for (int r = 0; r < 4; ++r) wacc = mfma_f64(kv[r], swb[(t * 16 + 4 * r + lq) * WST + lr], wacc);
    }
    if (more) store_slab(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // k(x, a_i): one more tile, D[query lq + 4 r][point lr]
  double kxa[4], hq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) hq[r] = shq[wave * 16 + lq + 4 * r];
  {
    d4_t c = {0.0, 0.0, 0.0, 0.0};
    double bf[KSTEPS];
#pragma unroll
    for (int k4 = 0; k4 < KSTEPS; ++k4) bf[k4] = sxa[lr * stride + lq + 4 * k4];
#pragma unroll
    for (int k4 = 0; k4 < KSTEPS; ++k4) c = mfma_f64(qf[k4], bf[k4], c);
    const double hk = sha[lr];
    double arg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) arg[r] = (c[r] - hq[r]) - hk;
    cov_nonpos4<KERN>(arg, stab, kxa);
  }

  if (column) {  // the columns k(X, a_i) over the observation rows (0 in the padding)
    if (lr < n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t g = qbase + wave * 16 + lq + 4 * r;
        if (g < Npad) p.kcol[((int64_t)lr * S + s) * Npad + g] = (g < N) ? kxa[r] : 0.0;
      }
    }
    return;
  }

  const double al = p.al[s * KL + lr];
  const long long arow = lr < n ? p.arows[lr] : -1;
  const double *mu = p.mu + s * Mtotal, *var = p.var + s * Mtotal;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t g = qbase + wave * 16 + lq + 4 * r;
    const int64_t gc = g < Mtotal ? g : Mtotal - 1;
    const double m = mu[gc], vr = var[gc];
    const double t = vr + tnoise;
    const double rs = sqrt(t);
    const double b = (kxa[r] - wacc[r]) / rs, b0 = vr / rs;
    const unsigned hit = (unsigned)(__ballot(arow == gc) >> (lane & 48)) & 0xffffu;  // is the query a row of A (by index)
    const bool own = hit == 0u;
    double v = kg_envelope(al, b, n, m, b0, own, lane);
    if (t == 0.0) v = 0.0;
    if (vr != vr || vr < 0.0 || m != m) v = __builtin_nan("");
    if (g < Mtotal) {
      if (lr == 0) p.v[s * Mtotal + g] = v;
      if (p.slopes) {
        double *sl = p.slopes + (s * Mtotal + g) * (n + 1);
        if (lr == 0) sl[0] = own ? b0 : __builtin_nan("");
        if (lr < n) sl[1 + lr] = b;
      }
    }
  }
}

size_t kg_lds_bytes(int dpad) {
  const int KO = kg_slab(dpad);
  const size_t r0 = (size_t)(KQ > 2 * KO ? KQ : 2 * KO) * (dpad + 1);
  return sizeof(double) * (r0 + 2 * KO + 2 * KO * WST + KQ + 128 + KL * (dpad + 1) + KL);
}

int launch_kg(b7_ctx *c, int S, const KgPass &p, bool column) {
  PhaseScope ps(c, column ? "kg_cols" : "kg");
  return ksx_for_class(c, "knowledge-gradient kernel", [&](auto cls) {
    using C = decltype(cls);
    const size_t lds = kg_lds_bytes(C::DPAD);
    auto kern = kg_kernel<C::DPAD, C::KERN>;
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t blocks = column ? c->Npad / KQ : (p.rows + KQ - 1) / KQ;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, 1, S), dim3(256), lds, c->stream, p, c->dfit, c->Npad, c->N, column ? 1 : 0);
    B7_HIP(c, hipGetLastError());
    return B7_OK;
  });
}

// ---- the small kernels around it -------------------------------------------------------------------------------------------
struct KgRows { long long row[KL]; };

// pick j of A: the lowest (1/S) sum_s mu_s over the rows not taken by picks 0 .. j-1; a lower marginal mean wins, then the lower
// index; a NaN counts as +inf, so n <= M rows are always found (argbest.h: OrderMinNanInf over this loader)
struct KgMeanLoad {
  const double *mu;  // [S][M]
  int S;
  long long M;
  __device__ __forceinline__ double operator()(long long g) const {
    double m = mu[g];
    for (int s = 1; s < S; ++s) m += mu[(long long)s * M + g];
    return m / (double)S;
  }
};
// the caller's rows: they travel as a kernel argument (no staging copy)
__global__ void kg_rows_set_kernel(KgRows r, int n, long long *__restrict__ rows) {
  if ((int)threadIdx.x < n) rows[threadIdx.x] = r.row[threadIdx.x];
}

// per sample (block): the points of A scaled as prep_obs_kernel scales an observation -- z .* w, and (sum z^2 w)/2 in ascending
// k --, and alpha_i = mu_s(a_i); zeros, 1e300 and 0 in the padding
__global__ void __launch_bounds__(256) kg_points_kernel(const double *__restrict__ grid, int d, int dpad, const long long *__restrict__ rows, int n,
                                                        const double *__restrict__ w, const double *__restrict__ mu, int64_t M,
                                                        double *__restrict__ sa, double *__restrict__ ha, double *__restrict__ al) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const double *ws = w + (int64_t)s * dpad;
  for (int e = tid; e < KL * dpad; e += 256) {
    const int i = e / dpad, k = e % dpad;
    sa[(int64_t)s * KL * dpad + e] = (i < n && k < d) ? grid[rows[i] * d + k] * ws[k] : 0.0;
  }
  if (tid < KL) {
    double a = 0.0;
    if (tid < n)
      for (int k = 0; k < d; ++k) {
        const double z = grid[rows[tid] * d + k];
        a += (z * z) * ws[k];
      }
    ha[s * KL + tid] = tid < n ? 0.5 * a : 1e300;
    al[s * KL + tid] = tid < n ? mu[(int64_t)s * M + rows[tid]] : 0.0;
  }
}

// acc[g] = v[0][g] + v[1][g] + ..: the samples in order (score:add x S; score:div is the finish kernel's)
__global__ void __launch_bounds__(256) kg_fold_kernel(const double *__restrict__ v, int S, int64_t M, double *__restrict__ acc) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < M; g += (int64_t)gridDim.x * 256) {
    double a = v[g];
    for (int s = 1; s < S; ++s) a += v[(int64_t)s * M + g];
    acc[g] = a;
  }
}

// b7_kg_compute: one input row per 16-lane row, column 0 its own line
__global__ void __launch_bounds__(256) kg_compute_kernel(const double *__restrict__ alpha, const double *__restrict__ b, int64_t M1, int L,
                                                         double *__restrict__ out) {
  const int lane = threadIdx.x & 63, lr = lane & 15;
  const int64_t q = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int64_t g = q < M1 ? q : M1 - 1;
  const int n = L - 1;
  const bool live = lr < n;
  const double a = live ? alpha[g * L + 1 + lr] : 0.0, bb = live ? b[g * L + 1 + lr] : 0.0;
  const double a0 = alpha[g * L], b0 = b[g * L];
  const double v = kg_envelope(a, bb, n, a0, b0, b0 == b0, lane);
  if (lr == 0 && q < M1) out[q] = v;
}

// the arrays of a call, carved out of c->kg and c->kgvec
struct KgState {
  double *mu, *var, *v;                      // [S][M] each
  double *kcol, *W, *par, *sa, *ha, *al;     // [KL][S][Npad] x 2, [S][2], [S][KL][dpad], [S][KL] x 2
  long long *rows;                           // [KL]
  ArgBest *part;                             // [nblk]
  int nblk;
};

int kg_state(b7_ctx *c, int S, KgState *st) {
  const size_t SM = (size_t)S * c->M, col = (size_t)KL * S * c->Npad;
  st->nblk = argbest_blocks(c->M);
  B7_TRY(b7_ensure(c, c->kg, sizeof(double) * 3 * SM));
  B7_TRY(b7_ensure(c, c->kgvec, sizeof(double) * (2 * col + 2 * (size_t)S + (size_t)S * KL * (c->dpad + 2) + KL + 2 * (size_t)st->nblk)));
  B7_TRY(b7_pin_ensure(c, c->pin_kg, sizeof(double) * 2 * (size_t)S, false));
  st->mu = (double *)c->kg.p, st->var = st->mu + SM, st->v = st->var + SM;
  st->kcol = (double *)c->kgvec.p, st->W = st->kcol + col, st->par = st->W + col, st->sa = st->par + 2 * (size_t)S;
  st->ha = st->sa + (size_t)S * KL * c->dpad, st->al = st->ha + (size_t)S * KL;
  st->rows = reinterpret_cast<long long *>(st->al + (size_t)S * KL);
  st->part = reinterpret_cast<ArgBest *>(st->rows + KL);
  return B7_OK;
}

// Everything behind the fits and posteriors of a nomination, enqueued: A, its columns, W, the pass over the grid, the fold onto
// the accumulator.  jit: what a redo added to each sample's diagonal (null: nothing).  rows0 (nullable): the caller's rows, 0-based
int kg_enqueue(b7_ctx *c, int S, const b7_hyp *hyps, const double *jit, int n, const KgRows *rows0, const BelKeep &keep, const KgState &st) {
  const int64_t M = c->M;
  const int np = c->Npad;
  double *par_host = static_cast<double *>(c->pin_kg.host);
  for (int s = 0; s < S; ++s) {
    par_host[2 * s] = hyps[s].amp;
    par_host[2 * s + 1] = hyps[s].noise + (jit && jit[s] > 0.0 ? jit[s] : 0.0);  // what went on the diagonal of the K that was factored
  }
  B7_HIP(c, hipMemcpyAsync(st.par, par_host, sizeof(double) * 2 * (size_t)S, hipMemcpyHostToDevice, c->stream));
  const double *grid = (const double *)c->grid[c->grid_cur].p;
  {
    PhaseScope ps(c, "kg_rows");
    if (rows0) {
      hipLaunchKernelGGL(kg_rows_set_kernel, dim3(1), dim3(64), 0, c->stream, *rows0, n, st.rows);
    } else {
      for (int j = 0; j < n; ++j)
        launch_argbest<OrderMinNanInf>(c->stream, KgMeanLoad{st.mu, S, (long long)M}, (long long)M, st.nblk, st.part, j, st.rows, (double *)nullptr);
    }
    hipLaunchKernelGGL(kg_points_kernel, dim3(S), dim3(256), 0, c->stream, grid, c->d, c->dpad, (const long long *)st.rows, n, keep.fits.w,
                       (const double *)st.mu, M, st.sa, st.ha, st.al);
    B7_HIP(c, hipGetLastError());
  }
  KgPass p;
  p.w = keep.fits.w, p.zsc = keep.fits.zsc, p.zss = keep.fits.zss;
  p.W = st.W, p.par = st.par, p.sa = st.sa, p.ha = st.ha, p.al = st.al, p.arows = st.rows;
  p.mu = st.mu, p.var = st.var, p.kcol = st.kcol, p.v = st.v, p.n = n;
  p.slopes = c->kg_trace_on ? (double *)c->kg_slopes.p : nullptr;
  p.xq = (const double *)c->xobs.p, p.rows = c->N;
  B7_TRY(launch_kg(c, S, p, true));
  for (int i = 0; i < n; ++i)
    B7_TRY(launch_alpha_batch(c, S, keep.fits.Linv, st.kcol + (size_t)i * S * np, st.W + (size_t)i * S * np));
  p.xq = grid, p.rows = M;
  B7_TRY(launch_kg(c, S, p, false));
  {
    PhaseScope ps(c, "kg_fold");
    B7_TRY(acc_write_zeros(c));  // the accumulator is declared written; the fold then writes every row of it
    hipLaunchKernelGGL(kg_fold_kernel, dim3(st.nblk), dim3(256), 0, c->stream, (const double *)st.v, S, M, (double *)c->acc.p);
    B7_HIP(c, hipGetLastError());
  }
  return B7_OK;
}

}  // namespace

extern "C" {

int b7_kg_nominate(b7_ctx *c, int S, const b7_hyp *hyps, int n, const int64_t *rows1, double *best_val, int64_t *best_idx1,
                   double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "kg_nominate: this context belongs to a group (the knowledge gradient over a sharded grid is not built)");
  if (n < 1 || n > B7_KG_MAX_POINTS) return b7_fail(c, B7_ERR_INVALID, "kg_nominate: n = %d discretisation points not in [1, %d]", n, B7_KG_MAX_POINTS);
  if (S < 1) return b7_fail(c, B7_ERR_INVALID, "kg_nominate: S = %d hyper samples (at least one)", S);
  if (!hyps || !best_val || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "kg_nominate: NULL argument (hyps, best_val and best_idx1 are needed)");
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "kg_nominate: a communicator of %d ranks (the knowledge gradient over a sharded grid is not built)", c->comm_world);
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "kg_nominate: no resident data (call b7_gp_set_data first)");
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "kg_nominate: no candidate grid on this context");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "kg_nominate: %d response columns (one is built)", c->ycols);
  if (c->opts.var_with_noise || c->opts.var_clamp)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "kg_nominate: the slopes are made of the latent variance (var_with_noise / var_clamp are set)");
  if (n > c->M) return b7_fail(c, B7_ERR_INVALID, "kg_nominate: n = %d exceeds the grid's %lld rows", n, (long long)c->M);
  KgRows rows0;
  if (rows1)
    for (int i = 0; i < n; ++i) {
      if (rows1[i] < 1 || rows1[i] > c->M)
        return b7_fail(c, B7_ERR_INVALID, "kg_nominate: rows1[%d] = %lld is not a row of the grid (1..%lld)", i, (long long)rows1[i], (long long)c->M);
      for (int k = 0; k < i; ++k)
        if (rows1[k] == rows1[i]) return b7_fail(c, B7_ERR_INVALID, "kg_nominate: row %lld is named twice (rows1[%d] and rows1[%d])", (long long)rows1[i], k, i);
      rows0.row[i] = rows1[i] - 1;
    }
  // the fits and posteriors are b7_eval_nominate's, asked for through a score that needs no f_min; its values are not used
  const b7_score_spec spec{B7_SCORE_CB, 0.0, 0, 1.0, nullptr};
  B7_TRY(eval_validate(c, S, hyps, &spec, 0));

  B7_HIP(c, hipSetDevice(c->device));
  c->kg_valid = false;
  KgState st;
  B7_TRY(kg_state(c, S, &st));
  if (c->kg_trace_on) B7_TRY(b7_ensure(c, c->kg_slopes, sizeof(double) * (size_t)S * c->M * (n + 1)));
  std::vector<double> jit(S, 0.0);
  if (jitter_out) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out) std::fill(info_out, info_out + S, 0);
  BelKeep keep;
  keep.mu = st.mu, keep.var = st.var;
  const KgRows *rp = rows1 ? &rows0 : nullptr;
  B7_TRY(nominate_run(
      c, "kg_nominate", B7_OK, 0, (double)S,
      [&](ScoreParams *pend) {
        ScoreParams unused;  // the small regime leaves its score:add pending: it is never launched
        B7_TRY(eval_enqueue(c, S, hyps, &spec, &unused, &keep));
        *pend = ScoreParams();
        return kg_enqueue(c, S, hyps, nullptr, n, rp, keep, st);
      },
      [&]() { return reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, true); },
      [&]() {
        B7_TRY(eval_redo(c, S, hyps, &spec, jit.data(), info_out, &keep));
        return kg_enqueue(c, S, hyps, jit.data(), n, rp, keep, st);
      },
      best_val, best_idx1));
  if (jitter_out) memcpy(jitter_out, jit.data(), sizeof(double) * S);
  c->fitted = false;  // the context's own fit slot holds none of the samples, as after b7_eval_nominate
  c->predicted = false;
  c->kg_valid = true;
  c->kg_S = S, c->kg_n = n, c->kg_M = c->M, c->kg_traced = c->kg_trace_on;
  c->kg_al_off = (size_t)(st.al - (double *)c->kgvec.p);
  return B7_OK;
}

int b7_kg_trace_enable(b7_ctx *c, int on) {
  if (!c) return B7_ERR_INVALID;
  c->kg_trace_on = on != 0;
  return B7_OK;
}

int b7_kg_last(b7_ctx *c, int64_t *rows1, double *alpha, double *slopes, double *values, double *own_alpha) {
  if (!c) return B7_ERR_INVALID;
  if (!c->kg_valid) return b7_fail(c, B7_ERR_STATE, "kg_last: no successful b7_kg_nominate on this context");
  if (slopes && !c->kg_traced) return b7_fail(c, B7_ERR_STATE, "kg_last: the last b7_kg_nominate kept no slopes (b7_kg_trace_enable before it)");
  B7_HIP(c, hipSetDevice(c->device));
  const int S = c->kg_S, n = c->kg_n;
  const size_t SM = (size_t)S * c->kg_M;
  // the layout kg_state made for that call (a later call lays the buffers out anew)
  const double *mu = (const double *)c->kg.p, *v = mu + 2 * SM;
  const double *al = (const double *)c->kgvec.p + c->kg_al_off;
  const long long *rows = reinterpret_cast<const long long *>(al + (size_t)S * KL);
  long long rh[KL];
  std::vector<double> ah((size_t)S * KL);
  B7_HIP(c, hipMemcpyAsync(rh, rows, sizeof(long long) * KL, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(ah.data(), al, sizeof(double) * (size_t)S * KL, hipMemcpyDeviceToHost, c->stream));
  if (slopes) B7_HIP(c, hipMemcpyAsync(slopes, c->kg_slopes.p, sizeof(double) * SM * (size_t)(n + 1), hipMemcpyDeviceToHost, c->stream));
  if (values) B7_HIP(c, hipMemcpyAsync(values, v, sizeof(double) * SM, hipMemcpyDeviceToHost, c->stream));
  if (own_alpha) B7_HIP(c, hipMemcpyAsync(own_alpha, mu, sizeof(double) * SM, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) {
    if (rows1) rows1[i] = rh[i] + 1;
    if (alpha)
      for (int s = 0; s < S; ++s) alpha[(size_t)s * n + i] = ah[(size_t)s * KL + i];
  }
  return B7_OK;
}

int b7_kg_compute(b7_ctx *c, int64_t M1, int L, const double *alpha, const double *b, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M1 < 0 || L < 1 || L > B7_KG_MAX_POINTS + 1 || (M1 > 0 && (!alpha || !b || !out)))
    return b7_fail(c, B7_ERR_INVALID, "kg_compute: bad arguments (M1 >= 0, L in 1..%d, arrays required)", B7_KG_MAX_POINTS + 1);
  if (M1 == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t ML = (size_t)M1 * L;
  B7_TRY(b7_ensure(c, c->kg_user, sizeof(double) * (2 * ML + (size_t)M1)));  // a buffer of its own: the last nomination's arrays stay
  double *ad = (double *)c->kg_user.p, *bd = ad + ML, *od = bd + ML;
  B7_HIP(c, hipMemcpyAsync(ad, alpha, sizeof(double) * ML, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(bd, b, sizeof(double) * ML, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(kg_compute_kernel, dim3((unsigned)((M1 + 15) / 16)), dim3(256), 0, c->stream, (const double *)ad, (const double *)bd, M1, L, od);
  B7_HIP(c, hipGetLastError());
  B7_HIP(c, hipMemcpyAsync(out, od, sizeof(double) * (size_t)M1, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays are consumed
  return B7_OK;
}

#ifdef B7_DIAG
// diagnostic build only: the columns k_s(X, a_i) and W_s[:, i] = inv(K_s) k_s(X, a_i) of the last b7_kg_nominate, [KL][S][Npad] each,
// as they stay resident in c->kgvec (kg_state lays them out first)
int b7dbg_kg_operands(b7_ctx *c, double *kcol_host, double *W_host) {
  if (!c || !c->kg_valid || !c->kgvec.p) return B7_ERR_INVALID;
  const size_t col = (size_t)KL * c->kg_S * c->Npad;
  if (c->kgvec.cap < sizeof(double) * 2 * col) return B7_ERR_INVALID;
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (kcol_host) B7_HIP(c, hipMemcpy(kcol_host, c->kgvec.p, sizeof(double) * col, hipMemcpyDeviceToHost));
  if (W_host) B7_HIP(c, hipMemcpy(W_host, (const double *)c->kgvec.p + col, sizeof(double) * col, hipMemcpyDeviceToHost));
  return B7_OK;
}
#endif

}  // extern "C"

// Thompson sampling: q nominees from q pathwise (decoupled) posterior samples -- b7_ts_nominate, b7_rff_compute.
//
// No counterpart in the reference.  A posterior sample path (Wilson, Borovitskiy, Terenin, Mostowsky, Deisenroth, ICML 2020) is
//   f_j(x) = m + phi(x)' w_j + K(x, X) v_j,        v_j = inv(K) (y - m - Phi(X) w_j - eps_j)
// with phi(x)[f] = sqrt(2 amp / F) cos(Omega[f] . x + phase[f]) F random Fourier features of the prior, w_j ~ N(0, I) and
// eps_j ~ N(0, noise I).  The update term m + K(x, X) v_j is the posterior mean of a fit whose response columns are the
// pseudo-responses y - Phi(X) w_j - eps_j: the multi-column fit and mean this library already has (launch_alpha, launch_ksx,
// launch_mean_multi).  New here is the prior term over the whole grid, rff_kernel:
//   out[i][p] = base[i][p] + sum_f W[f][p] cos(sum_k X[i][k] Omega[f][k] + phase[f])          i < M, p < q <= 16, f < F
// Phi (M x F) is never stored.  The fragment chain (gemm_f64.h's maps; the observation kpost_small.hip rests on): per 16
// features and 16 candidates
//   1. D = Omega_chunk (A operand: row f, k) x X' (B operand: k, column c), DPAD / 4 MFMAs; D[f][c] sits at lane
//      16 (f mod 4) + c, register f / 4;
//   2. that register, after + phase[f] and the cosine in place, is a valid B operand of a second product with k = feature
//      (MFMA step r covers the features 4 r .. 4 r + 3);
//   3. Out[p][c] += W'[p][f] cosD[f][c], W' as the A operand, 4 MFMAs: the q <= 16 paths pad to exactly one tile;
//   4. out[c][p] is stored once, after the last chunk.
// No LDS, no transposition, one summation order over the features whatever M is.  Omega and W reach the kernel already in
// fragment order and zero padded (rff_pack_kernel), so every operand load is one coalesced 8-byte read per lane, rows beyond M
// are staged as zeros and no padding can make a NaN.  The fp64 MFMA and the fp64 VALU share the same units (gemm_f64.h), so
// the kernel's bound is the SUM of its MFMA and its VALU issue: per tile of 16 x 16, DPAD / 4 + 4 MFMAs of 64 cycles and four
// cosines per lane (rff_cos below: 29 VALU instructions with its phase add, against ocml's ~100 with its large-argument path).
//
// The draws (counter_rng.h states the counter layout): ARD-SE has Omega[f][k] = z / sqrt(lenscale_sq[k]); ARD Matern-5/2 has the
// multivariate t with 5 degrees of freedom, Omega[f][k] = z sqrt(5 / u_f) / sqrt(lenscale_sq[k]), u_f the sum of five squared
// normals.  The basis (z, u, phase) is one per call and shared by its paths -- only the lengthscales of path j's hyper sample,
// j mod S, enter its Omega --; weight and eps are path j's own.  All of it depends on (seed, j) alone.
//
// Out of scope: sharded grids and groups (the q arg-mins would ride the existing all-reduce, but no world > 1 has run on
// hardware), more than one response column, a one-launch variant for N <= 128, and any change to the existing scores or the
// believer batch.  The Bayesian-linear head has its own entry, b7_blr_ts_nominate (blr_ts.hip), which shares the arg-mins below.
#include <math.h>
#include <string.h>

#include <vector>

#include "b7_internal.h"
#include "counter_rng.h"
#include "gemm_f64.h"

namespace {

constexpr int RT = 2;            // 16-candidate tiles per wave: an Omega / W fragment is loaded once for both
constexpr int RROWS = 4 * 16 * RT;  // candidate rows per block of four waves

// cos(x) for |x| < 2^30: n = rint(x 2/pi), r = x - n pi/2 by a two-term Cody-Waite reduction whose products the fma keeps exact
// (|r| <= pi/4 to 2^-54 absolute while n pi/2's low word matters, i.e. far beyond the |x| of a few thousand that unit-cube
// inputs over lengthscales >= 1e-3 give), then fdlibm's kernel polynomials on [-pi/4, pi/4] (both evaluated, one selected: 13
// fmas against the 14 selects of choosing coefficients) and the quadrant's sign.  Below 1 ulp of the result near |x| <= pi/4,
// ~1.2e-16 absolute elsewhere.  NaN and Inf give NaN.
__device__ __forceinline__ double rff_cos(double x) {
  const double n = __builtin_rint(x * 6.36619772367581382433e-01);
  double r = __builtin_fma(-n, 1.57079632679489655800e+00, x);
  r = __builtin_fma(-n, 6.12323399573676603587e-17, r);
  const double z = r * r;
  double ps = 1.58969099521155010221e-10;
  ps = __builtin_fma(ps, z, -2.50507602534068634195e-08);
  ps = __builtin_fma(ps, z, 2.75573137070700676789e-06);
  ps = __builtin_fma(ps, z, -1.98412698298579493134e-04);
  ps = __builtin_fma(ps, z, 8.33333333332248946124e-03);
  ps = __builtin_fma(ps, z, -1.66666666666666324348e-01);
  const double sn = __builtin_fma(z * r, ps, r);
  double pc = -1.13596475577881948265e-11;
  pc = __builtin_fma(pc, z, 2.08757232129817482790e-09);
  pc = __builtin_fma(pc, z, -2.75573143513906633035e-07);
  pc = __builtin_fma(pc, z, 2.48015872894767294178e-05);
  pc = __builtin_fma(pc, z, -1.38888888888741095749e-03);
  pc = __builtin_fma(pc, z, 4.16666666666666019037e-02);
  pc = __builtin_fma(pc, z, -0.5);
  const double cs = __builtin_fma(pc, z, 1.0);
  // cos(r + n pi/2): n mod 4 = 0: cos r, 1: -sin r, 2: -cos r, 3: sin r
  const int k = (int)n;
  double v = (k & 1) ? sn : cs;
  return ((k + 1) & 2) ? -v : v;
}

// Omega (F x d, row-major) and W (F x ldw, qn <= 16 live columns) into the fragment order rff_kernel reads, zero padded:
//   omf[(ch KS + k4) 64 + lane] = Omega[16 ch + (lane & 15)][4 k4 + (lane >> 4)]        KS = DPAD / 4
//   wf[(ch 4 + r) 64 + lane]    = scale W[16 ch + 4 r + (lane >> 4)][col0 + (lane & 15) cstride]
__global__ void __launch_bounds__(256) rff_pack_kernel(const double *__restrict__ omega, int F, int d, int dpad, const double *__restrict__ W,
                                                       int64_t ldw, int64_t col0, int64_t cstride, int qn, double scale,
                                                       double *__restrict__ omf, double *__restrict__ wf) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int KS = dpad / 4;
  const int64_t nom = (int64_t)F * dpad;
  if (e < nom) {
    const int lane = (int)(e & 63);
    const int64_t t = e >> 6;
    const int k4 = (int)(t % KS), f = (int)(t / KS) * 16 + (lane & 15), k = 4 * k4 + (lane >> 4);
    omf[e] = k < d ? omega[(int64_t)f * d + k] : 0.0;
  } else if (e < nom + (int64_t)F * 16) {
    const int64_t w = e - nom;
    const int lane = (int)(w & 63);
    const int64_t t = w >> 6;
    const int r = (int)(t & 3), f = (int)(t >> 2) * 16 + 4 * r + (lane >> 4), p = lane & 15;
    wf[w] = p < qn ? scale * W[(int64_t)f * ldw + col0 + p * cstride] : 0.0;
  }
}

// out[i][ocol0 + p ostride] = (base ? base[i][p] : 0) + sum_f W[f][p] cos(Omega[f] . X[i] + phase[f]),  i < M, p < qn
template <int DPAD>
__global__ void __launch_bounds__(256) rff_kernel(const double *__restrict__ X, int64_t M, int d, const double *__restrict__ omf,
                                                  const double *__restrict__ phase, const double *__restrict__ wf, int nchunk,
                                                  const double *__restrict__ base, int ldb, double *__restrict__ out, int ldo, int ocol0,
                                                  int ostride, int qn) {
  constexpr int KS = DPAD / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * RROWS + wave * (16 * RT);
  if (row0 >= M) return;  // wave-uniform; the kernel has no barrier

  // B fragments of X': candidate (row0 + 16 t + lr), k = 4 k4 + lq; zeros beyond M and d
  double xb[RT][KS];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t g = row0 + 16 * t + lr;
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) {
      const int k = 4 * k4 + lq;
      xb[t][k4] = (g < M && k < d) ? X[g * d + k] : 0.0;
    }
  }
  d4_t acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};

  double a[KS], ph[4], wv[4];  // the chunk in flight, loaded one chunk ahead of its use
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) a[k4] = omf[((int64_t)ch * KS + k4) * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ph[r] = phase[ch * 16 + lq + 4 * r];
      wv[r] = wf[((int64_t)ch * 4 + r) * 64 + lane];
    }
  };
  load_chunk(0);
  for (int ch = 0; ch < nchunk; ++ch) {
    double ca[KS], cph[4], cw[4];
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) ca[k4] = a[k4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cph[r] = ph[r], cw[r] = wv[r];
    if (ch + 1 < nchunk) load_chunk(ch + 1);
    d4_t D[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      D[t] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k4 = 0; k4 < KS; ++k4) D[t] = mfma_f64(ca[k4], xb[t][k4], D[t]);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) D[t][r] = rff_cos(D[t][r] + cph[r]);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t] = mfma_f64(cw[r], D[t][r], acc[t]);
    }
  }
  // acc[t][r]: path p = lq + 4 r, candidate row0 + 16 t + lr
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t g = row0 + 16 * t + lr;
    if (g >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = lq + 4 * r;
      if (p < qn) out[g * ldo + ocol0 + (int64_t)p * ostride] = (base ? base[g * ldb + p] : 0.0) + acc[t][r];
    }
  }
}

// ---- the draws ----------------------------------------------------------------------------------------------------------
// omega[f][k] (F x d) under one hyper sample's inverse lengthscales; phase[f] alongside when asked for (it does not depend on them)
__global__ void __launch_bounds__(256) ts_basis_kernel(uint64_t key, int F, int d, int matern, const double *__restrict__ inv_ls,
                                                       double *__restrict__ omega, double *__restrict__ phase) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)F * d) return;
  const int f = (int)(e / d), k = (int)(e - (int64_t)f * d);
  double v = counter_normal(key, (uint64_t)f * 128 + (uint64_t)k);
  if (matern) {
    double u = 0.0;
    for (int i = 0; i < 5; ++i) {
      const double g = counter_normal(key, (uint64_t)f * 128 + 96 + (uint64_t)i);
      u += g * g;
    }
    v = v * sqrt(5.0 / u);
  }
  omega[e] = v * inv_ls[k];
  if (phase && k == 0) phase[f] = 6.283185307179586476925 * counter_uniform(key, (uint64_t)f * 128 + 101);
}

// weight[j][f] ~ N(0,1) (q x F) and z_eps[j][i] ~ N(0,1) (q x N; eps = sqrt(noise) z_eps is formed with the pseudo-responses)
__global__ void __launch_bounds__(256) ts_path_draws_kernel(uint64_t seed, int q, int F, int N, double *__restrict__ weight,
                                                            double *__restrict__ zeps) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)F + N;
  if (e >= per * q) return;
  const int j = (int)(e / per);
  const int64_t i = e - (int64_t)j * per;
  const uint64_t key = counter_key(seed, 1 + (uint64_t)j);
  if (i < F)
    weight[(int64_t)j * F + i] = counter_normal(key, (uint64_t)i);
  else
    zeps[(int64_t)j * N + (i - F)] = counter_normal(key, 4096 + (uint64_t)(i - F));
}

// eps[j][i] = sqrt(noise) z_eps[j][i] in place for the sample's paths j = s + S p, and the pseudo-responses
// ycols[i][p] = y[i] - phiw[i][p] - eps[j][i]
__global__ void __launch_bounds__(256) ts_pseudo_kernel(const double *__restrict__ y, const double *__restrict__ phiw, double *__restrict__ eps,
                                                        int N, int qs, int s, int S, double sd_noise, double *__restrict__ ycols) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * qs) return;
  const int i = e / qs, p = e - i * qs;
  double *ej = eps + (int64_t)(s + S * p) * N + i;
  const double ev = sd_noise * *ej;
  *ej = ev;
  ycols[e] = (y[i] - phiw[e]) - ev;
}

template <int DPAD>
void rff_launch_class(b7_ctx *c, const double *X, int64_t M, int d, const double *omf, const double *phase, const double *wf, int F,
                      const double *base, int ldb, double *out, int ldo, int ocol0, int ostride, int qn) {
  hipLaunchKernelGGL(rff_kernel<DPAD>, dim3((unsigned)((M + RROWS - 1) / RROWS)), dim3(256), 0, c->stream, X, M, d, omf, phase, wf, F / 16,
                     base, ldb, out, ldo, ocol0, ostride, qn);
}

int launch_rff(b7_ctx *c, const double *X, int64_t M, int d, const double *omf, const double *phase, const double *wf, int F,
               const double *base, int ldb, double *out, int ldo, int ocol0, int ostride, int qn) {
  PhaseScope ps(c, "rff");
  if (M <= 0) return B7_OK;
  switch (rff_dpad(d)) {
    case 8: rff_launch_class<8>(c, X, M, d, omf, phase, wf, F, base, ldb, out, ldo, ocol0, ostride, qn); break;
    case 16: rff_launch_class<16>(c, X, M, d, omf, phase, wf, F, base, ldb, out, ldo, ocol0, ostride, qn); break;
    case 32: rff_launch_class<32>(c, X, M, d, omf, phase, wf, F, base, ldb, out, ldo, ocol0, ostride, qn); break;
    case 64: rff_launch_class<64>(c, X, M, d, omf, phase, wf, F, base, ldb, out, ldo, ocol0, ostride, qn); break;
    default: rff_launch_class<96>(c, X, M, d, omf, phase, wf, F, base, ldb, out, ldo, ocol0, ostride, qn); break;
  }
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int launch_rff_pack(b7_ctx *c, const double *omega, int F, int d, const double *W, int64_t ldw, int64_t col0, int64_t cstride, int qn,
                    double scale, double *omf, double *wf) {
  const int dpad = rff_dpad(d);
  const int64_t total = (int64_t)F * (dpad + 16);
  hipLaunchKernelGGL(rff_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, omega, F, d, dpad, W, ldw, col0,
                     cstride, qn, scale, omf, wf);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// c->ts_draw: what b7_ts_last_draws reads back, laid out for (ns used hyper samples, q paths, F features, d dims, N observations)
struct TsDraws { double *omega, *phase, *weight, *eps; };  // [ns][F][d] | [F] | [q][F] | [q][N]
TsDraws ts_draws(const b7_ctx *c, int ns, int q, int F, int d, int N) {
  TsDraws t;
  t.omega = (double *)c->ts_draw.p;
  t.phase = t.omega + (size_t)ns * F * d;
  t.weight = t.phase + F;
  t.eps = t.weight + (size_t)q * F;
  (void)N;
  return t;
}

// the posterior mean of the context's current fit (c->ycols columns) over the resident grid into c->mu, without the variance
int ts_mean_over_grid(b7_ctx *c) {
  const int64_t M = c->M, chunk = predict_chunk(c, M), Mpad = round_up(M, B7_MROWS);
  B7_TRY(b7_ensure(c, c->ks, sizeof(double) * (size_t)chunk * c->Npad));
  const double *grid = (const double *)c->grid[c->grid_cur].p;
  for (int64_t row0 = 0; row0 < M; row0 += chunk) {
    const int64_t rows = Mpad - row0 < chunk ? Mpad - row0 : chunk;
    B7_TRY(launch_ksx(c, ctx_fit(c), grid, row0, rows, M, c->dfit, (double *)c->ks.p, (double *)c->mu.p, c->ycols));
    if (c->ycols > 1) B7_TRY(launch_mean_multi(c, ctx_fit(c), (const double *)c->ks.p, row0, rows, M, (double *)c->mu.p));
  }
  return B7_OK;
}

// c->ts_work: one hyper sample's operands, each piece on a 256-byte boundary (the multi-column mean reads alpha in 16-byte pairs):
// omf F dpad | wf 16 F | phiw N qmax | ycols np qmax | alpha np yldmax | resid np qmax | inv_ls d | pmin q | taken q | part 2 nblk
// Every hyper sample's alpha is kept (ns of them, sample s at alpha + s np yldmax): column p of sample s is v_j of path j = s + S p,
// which the refinement of the paths (ts_refine.hip, through ts_kept) and b7dbg_ts_alpha read.  ts_paths_core carves the buffer with
// this, once, and records where alpha, pmin, taken and part lie in c->ts: nobody else derives the layout.
void ts_work_layout(int F, int dpad, int N, int np, int qmax, int yldmax, int d, int q, int nblk, int ns, size_t off[11]) {
  const size_t nalpha = (size_t)ns;
  const size_t pieces[10] = {(size_t)F * dpad, 16 * (size_t)F, (size_t)N * qmax, (size_t)np * qmax, nalpha * np * yldmax, (size_t)np * qmax,
                             (size_t)d,        (size_t)q,      (size_t)q,        2 * (size_t)nblk};
  off[0] = 0;
  for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + (size_t)round_up((int64_t)pieces[i], 32);
}

// The context's response columns while a hyper sample's pseudo-responses are being fitted: put back on every way out.
struct YSwap {
  b7_ctx *c;
  DevBuf ybuf, alpha, resid;
  int ycols, yld;
  explicit YSwap(b7_ctx *c) : c(c), ybuf(c->ybuf), alpha(c->alpha), resid(c->resid), ycols(c->ycols), yld(c->yld) {}
  ~YSwap() {
    c->ybuf = ybuf, c->alpha = alpha, c->resid = resid, c->ycols = ycols, c->yld = yld;
    c->fitted = false;  // the context's own fit slot holds none of the samples
    c->predicted = false;
  }
};

}  // namespace

// ---- the arg-mins: path j's first minimum over the rows no earlier path of the call took; a NaN does not win (argbest.h) ----
int launch_ts_argmin(b7_ctx *c, const double *paths, int64_t M, int q, int j, double *pmin, long long *taken, ArgBest *part, int nblk) {
  launch_argbest<OrderMinNanLast>(c->stream, ArgLoadStrided{paths + j, q}, (long long)M, nblk, part, j, taken, pmin);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int launch_ts_argmins(b7_ctx *c, const double *paths, int64_t M, int q, double *pmin, long long *taken, ArgBest *part, int nblk) {
  PhaseScope ps(c, "ts_argmin");
  for (int j = 0; j < q; ++j) B7_TRY(launch_ts_argmin(c, paths, M, q, j, pmin, taken, part, nblk));
  return B7_OK;
}

// What the last GP paths left for their refinement: the draws and every path's v_j (b7_internal.h: TsKept)
int ts_kept(const b7_ctx *c, TsKept *k) {
  const TsPaths &t = c->ts;
  if (t.who != TS_GP) return B7_ERR_STATE;
  const TsDraws dr = ts_draws(c, t.ns, t.q, t.F, t.d, t.N);
  k->omega = dr.omega, k->phase = dr.phase, k->weight = dr.weight;
  k->alpha = t.alpha, k->alpha_stride = t.alpha_stride;
  k->ns = t.ns;
  return B7_OK;
}

namespace {

// The path half of a Thompson nomination, b7_ts_nominate's and b7_ts_paths' (`who` in the messages): validation, draws, one fit per
// hyper sample and the paths over the grid into c->ts_paths ([M][q]); c->ts records what they are and where their pieces lie.  null_out:
// an output of the entry's own is missing (answered in its place among the checks); what: the arguments the entry needs, for that message.
int ts_paths_core(b7_ctx *c, const char *who, bool null_out, const char *what, int S, const b7_hyp *hyps, int q, int F, uint64_t seed,
                  double *jitter_out, int *info_out) {
  if (c->group) return b7_fail(c, B7_ERR_STATE, "%s: this context belongs to a group (sharded Thompson sampling is not built)", who);
  if (q < 1 || q > B7_BATCH_MAX) return b7_fail(c, B7_ERR_INVALID, "%s: q = %d not in [1, %d]", who, q, B7_BATCH_MAX);
  if (F < 16 || F > B7_TS_MAX_FEATURES || F % 16)
    return b7_fail(c, B7_ERR_INVALID, "%s: F = %d features: a multiple of 16 in [16, %d]", who, F, B7_TS_MAX_FEATURES);
  if (S < 1) return b7_fail(c, B7_ERR_INVALID, "%s: S = %d hyper samples (at least one)", who, S);
  if (!hyps || null_out) return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (%s)", who, what);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: a communicator of %d ranks (sharded Thompson sampling is not built)", who, c->comm_world);
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "%s: no resident data (call b7_gp_set_data first)", who);
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "%s: no candidate grid on this context", who);
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: %d response columns (one is built)", who, c->ycols);
  if (c->d != c->dfit) return b7_fail(c, B7_ERR_INVALID, "%s: grid dims %d != data dims %d", who, c->d, c->dfit);
  if (q > c->M) return b7_fail(c, B7_ERR_INVALID, "%s: q = %d exceeds the grid's %lld rows", who, q, (long long)c->M);
  const int ns = S < q ? S : q, N = c->N, d = c->dfit, dpad = rff_dpad(d), np = c->Npad;
  for (int s = 0; s < ns; ++s) B7_TRY(check_hyp(c, &hyps[s], d));
  B7_HIP(c, hipSetDevice(c->device));
  const int64_t M = c->M;
  if (jitter_out) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out) std::fill(info_out, info_out + S, 0);
  TsPaths &t = c->ts;
  t.who = TS_NONE;
  t.hyp.resize((size_t)ns * (d + 3));  // the hyper samples the paths are drawn under, for the paths' refinement
  for (int s = 0; s < ns; ++s) {
    double *hs = &t.hyp[(size_t)s * (d + 3)];
    std::copy(hyps[s].lenscale_sq, hyps[s].lenscale_sq + d, hs);
    hs[d] = hyps[s].amp, hs[d + 1] = hyps[s].noise, hs[d + 2] = hyps[s].mean;
  }

  // device memory beyond the posterior's own: the paths (M x q), the draws, and the operands of one hyper sample
  const int qmax = (q + ns - 1) / ns, yldmax = qmax == 1 ? 1 : (int)round_up(qmax, 64);
  const int nblk = argbest_blocks(M);
  B7_TRY(b7_ensure(c, c->ts_paths, sizeof(double) * (size_t)M * q));
  B7_TRY(b7_ensure(c, c->ts_draw, sizeof(double) * ((size_t)ns * F * d + F + (size_t)q * F + (size_t)q * N)));
  size_t off[11];
  ts_work_layout(F, dpad, N, np, qmax, yldmax, d, q, nblk, ns, off);
  B7_TRY(b7_ensure(c, c->ts_work, sizeof(double) * off[10]));
  const TsDraws dr = ts_draws(c, ns, q, F, d, N);
  double *wk = (double *)c->ts_work.p;
  double *omf = wk + off[0], *wf = wk + off[1], *phiw = wk + off[2], *ycols = wk + off[3], *alpha = wk + off[4], *resid = wk + off[5];
  double *inv_ls = wk + off[6];
  double *paths = (double *)c->ts_paths.p;
  const double *grid = (const double *)c->grid[c->grid_cur].p;

  {
    const int64_t total = ((int64_t)F + N) * q;
    hipLaunchKernelGGL(ts_path_draws_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, seed, q, F, N, dr.weight, dr.eps);
    B7_HIP(c, hipGetLastError());
  }
  const uint64_t key0 = counter_key(seed, 0);
  std::vector<double> ils(d);
  {
    YSwap swap(c);
    for (int s = 0; s < ns; ++s) {
      const int qs = (q - s + S - 1) / S;  // the paths j = s, s + S, .. < q
      const b7_hyp &h = hyps[s];
      for (int k = 0; k < d; ++k) ils[k] = 1.0 / sqrt(h.lenscale_sq[k]);
      B7_HIP(c, hipMemcpyAsync(inv_ls, ils.data(), sizeof(double) * d, hipMemcpyHostToDevice, c->stream));
      B7_HIP(c, hipStreamSynchronize(c->stream));  // ils is reused by the next sample
      double *omega = dr.omega + (size_t)s * F * d;
      {
        PhaseScope ps(c, "ts_draws");
        hipLaunchKernelGGL(ts_basis_kernel, dim3((unsigned)(((int64_t)F * d + 255) / 256)), dim3(256), 0, c->stream, key0, F, d,
                           c->kernel == B7_KERNEL_MATERN52 ? 1 : 0, (const double *)inv_ls, omega, s == 0 ? dr.phase : (double *)nullptr);
        B7_HIP(c, hipGetLastError());
        // W[f][p] = sqrt(2 amp / F) weight[s + S p][f]: row f, leading dimension 1, column p at stride S F
        B7_TRY(launch_rff_pack(c, omega, F, d, dr.weight + (size_t)s * F, 1, 0, (int64_t)S * F, qs, sqrt(2.0 * h.amp / F), omf, wf));
      }
      // the pseudo-responses of this sample's paths, then one fit with those columns
      B7_TRY(launch_rff(c, (const double *)c->xobs.p, N, d, omf, dr.phase, wf, F, nullptr, 0, phiw, qs, 0, 1, qs));
      hipLaunchKernelGGL(ts_pseudo_kernel, dim3((unsigned)((N * qs + 255) / 256)), dim3(256), 0, c->stream, (const double *)swap.ybuf.p,
                         (const double *)phiw, dr.eps, N, qs, s, S, sqrt(h.noise), ycols);
      B7_HIP(c, hipGetLastError());
      double *alpha_s = alpha + (size_t)s * np * yldmax;
      c->ybuf.p = ycols, c->alpha.p = alpha_s, c->resid.p = resid;  // (capacities are not consulted while swapped: nothing regrows these)
      c->ycols = qs;
      c->yld = qs == 1 ? 1 : (int)round_up(qs, 64);
      double jit = 0.0;
      int info = 0;
      B7_TRY(fit_hyp_core(c, &h, nullptr, &jit, &info, false));
      if (jitter_out) jitter_out[s] = jit;
      if (info_out) info_out[s] = info;
      B7_TRY(b7_ensure(c, c->mu, sizeof(double) * (size_t)M * qs));
      B7_TRY(ts_mean_over_grid(c));
      // f_j = (m + K(x, X) v_j) + phi(x)' w_j into column j = s + S p of the paths
      B7_TRY(launch_rff(c, grid, M, d, omf, dr.phase, wf, F, (const double *)c->mu.p, qs, paths, q, s, S, qs));
    }
  }
  t.M = M, t.q = q, t.S = S, t.F = F, t.N = N, t.d = d, t.ns = ns;
  t.epoch = c->epoch;
  t.alpha = alpha, t.alpha_stride = (int64_t)np * yldmax;
  t.pmin = wk + off[7], t.taken = reinterpret_cast<long long *>(wk + off[8]), t.part = reinterpret_cast<ArgBest *>(wk + off[9]), t.nblk = nblk;
  t.who = TS_GP;
  return B7_OK;
}

#ifdef B7_DIAG
// b7dbg_argbest_loop's kernel: n <= 16 successive picks by ONE workgroup that calls block_best in a loop, a barrier ahead of every
// call, each pick leaving out the earlier ones
template <class Order>
__global__ void __launch_bounds__(256) dbg_argbest_loop_kernel(const double *__restrict__ v, long long M, int n, long long *__restrict__ taken,
                                                               double *__restrict__ val) {
  __shared__ ArgBest sh[4];
  long long ex[ARGBEST_MAX_EXCL];
  argbest_load_excl(nullptr, 0, ex);
  for (int p = 0; p < n; ++p) {
    ArgBest b{0.0, -1};
    for (long long r = threadIdx.x; r < M; r += 256) {
      const ArgBest cnd{v[r], r};
      if (argbest_excluded(ex, r) || (Order::skips_nan && cnd.v != cnd.v)) continue;
      if (Order()(cnd, b)) b = cnd;
    }
    __syncthreads();  // sh is free again
    b = block_best<Order>(b, sh);
#pragma unroll
    for (int e = 0; e < ARGBEST_MAX_EXCL; ++e) ex[e] = (e == p) ? b.i : ex[e];  // (ex stays in registers)
    if (threadIdx.x == 0) taken[p] = b.i, val[p] = b.v;
  }
}
// both diagnostic entries: values M | taken 32 | val 32 | part 2 x 1024 on b7_rff_compute's staging buffer
int dbg_argbest_run(b7_ctx *c, int order, const double *values, int64_t M, const long long *excl, int n, bool loop, double *val_out,
                    long long *row_out) {
  if (!c || !values || M < 1 || n < (loop ? 1 : 0) || n > ARGBEST_MAX_EXCL || (!loop && n > 0 && !excl) || !val_out || !row_out) return B7_ERR_INVALID;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t m = (size_t)round_up(M, 32);
  B7_TRY(b7_ensure(c, c->ts_user, sizeof(double) * (m + 64 + 2 * 1024)));
  double *vd = (double *)c->ts_user.p, *val = vd + m + 32;
  long long *taken = reinterpret_cast<long long *>(vd + m);
  B7_HIP(c, hipMemcpyAsync(vd, values, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  if (!loop && n > 0) B7_HIP(c, hipMemcpyAsync(taken, excl, sizeof(long long) * n, hipMemcpyHostToDevice, c->stream));
  auto run = [&](auto ord) {
    using Order = decltype(ord);
    if (loop) hipLaunchKernelGGL(dbg_argbest_loop_kernel<Order>, dim3(1), dim3(256), 0, c->stream, (const double *)vd, (long long)M, n, taken, val);
    else launch_argbest<Order>(c->stream, ArgLoadStrided{vd, 1}, (long long)M, argbest_blocks(M), reinterpret_cast<ArgBest *>(vd + m + 64), n, taken, val);
  };
  switch (order) {
    case 0: run(OrderMaxNanFirst()); break;
    case 1: run(OrderMinNanLast()); break;
    case 2: run(OrderMaxNoNan()); break;
    case 3: run(OrderMinNanInf()); break;
    case 4: run(OrderMin()); break;
    default: return B7_ERR_INVALID;
  }
  B7_HIP(c, hipGetLastError());
  const int k0 = loop ? 0 : n, cnt = loop ? n : 1;  // one pass leaves pick n_excl; the loop leaves picks 0 .. n - 1
  B7_HIP(c, hipMemcpyAsync(val_out, val + k0, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(row_out, taken + k0, sizeof(long long) * cnt, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}
#endif

}  // namespace

extern "C" {

int b7_ts_nominate(b7_ctx *c, int S, const b7_hyp *hyps, int q, int F, uint64_t seed, double *path_min, int64_t *best_idx1,
                   double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(ts_paths_core(c, "ts_nominate", !path_min || !best_idx1, "hyps, path_min and best_idx1 are needed", S, hyps, q, F, seed, jitter_out,
                       info_out));
  TsPaths &t = c->ts;
  t.who = TS_NONE;  // until the arg-mins have come back
  B7_TRY(launch_ts_argmins(c, (const double *)c->ts_paths.p, t.M, q, t.pmin, t.taken, t.part, t.nblk));
  long long tk[B7_BATCH_MAX];
  B7_HIP(c, hipMemcpyAsync(path_min, t.pmin, sizeof(double) * q, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(tk, t.taken, sizeof(long long) * q, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < q; ++j) best_idx1[j] = tk[j] + 1;
  t.who = TS_GP;
  return B7_OK;
}

int b7_ts_paths(b7_ctx *c, int S, const b7_hyp *hyps, int q, int F, uint64_t seed, double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(ts_paths_core(c, "ts_paths", false, "hyps is needed", S, hyps, q, F, seed, jitter_out, info_out));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the fits' reports (jitter_out, info_out) are complete and the paths stand
  return B7_OK;
}

int b7_ts_last_paths(b7_ctx *c, double *paths_host) {
  if (!c) return B7_ERR_INVALID;
  if (!paths_host) return b7_fail(c, B7_ERR_INVALID, "ts_last_paths: NULL argument");
  if (ts_state(c) == TS_STATE_NONE) return b7_fail(c, B7_ERR_STATE, "ts_last_paths: no successful b7_ts_nominate or b7_ts_paths on this context");
  B7_HIP(c, hipSetDevice(c->device));  // (stale paths are served too)
  B7_HIP(c, hipMemcpyAsync(paths_host, c->ts_paths.p, sizeof(double) * (size_t)c->ts.M * c->ts.q, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_ts_last_draws(b7_ctx *c, int path, double *omega, double *phase, double *weight, double *eps) {
  if (!c) return B7_ERR_INVALID;
  const TsPaths &t = c->ts;
  const int state = ts_state(c);
  if (state == TS_STATE_NONE) return b7_fail(c, B7_ERR_STATE, "ts_last_draws: no successful b7_ts_nominate or b7_ts_paths on this context");
  if (state == TS_STATE_BLR) return b7_fail(c, B7_ERR_STATE, "ts_last_draws: the last nomination was b7_blr_ts_nominate's (b7_blr_ts_last_draws reads its draws)");
  if (path < 0 || path >= t.q) return b7_fail(c, B7_ERR_INVALID, "ts_last_draws: path %d not in [0, %d)", path, t.q);
  B7_HIP(c, hipSetDevice(c->device));
  const int F = t.F, d = t.d, N = t.N;
  const TsDraws dr = ts_draws(c, t.ns, t.q, F, d, N);
  if (omega) B7_HIP(c, hipMemcpyAsync(omega, dr.omega + (size_t)(path % t.S) * F * d, sizeof(double) * (size_t)F * d, hipMemcpyDeviceToHost, c->stream));
  if (phase) B7_HIP(c, hipMemcpyAsync(phase, dr.phase, sizeof(double) * F, hipMemcpyDeviceToHost, c->stream));
  if (weight) B7_HIP(c, hipMemcpyAsync(weight, dr.weight + (size_t)path * F, sizeof(double) * F, hipMemcpyDeviceToHost, c->stream));
  if (eps) B7_HIP(c, hipMemcpyAsync(eps, dr.eps + (size_t)path * N, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

#ifdef B7_DIAG
// diagnostic build only: the alpha columns (N x qs, row-major; qs = the paths j = s, s + S, .. < q) of hyper sample s's
// pseudo-response fit in the last b7_ts_nominate; *qs_out (nullable) receives qs
int b7dbg_ts_alpha(b7_ctx *c, int s, double *out_host, int *qs_out) {
  if (!c || !out_host || c->ts.who != TS_GP || c->ts.N != c->N) return B7_ERR_INVALID;
  const TsPaths &t = c->ts;
  if (s < 0 || s >= t.ns) return B7_ERR_INVALID;
  const int qs = (t.q - s + t.S - 1) / t.S, yld = qs == 1 ? 1 : (int)round_up(qs, 64);
  const double *alpha = t.alpha + (size_t)s * t.alpha_stride;
  B7_HIP(c, hipStreamSynchronize(c->stream));
  B7_HIP(c, hipMemcpy2D(out_host, sizeof(double) * qs, alpha, sizeof(double) * yld, sizeof(double) * qs, t.N, hipMemcpyDeviceToHost));
  if (qs_out) *qs_out = qs;
  return B7_OK;
}

// diagnostic build only: argbest.h on the caller's values[M].  order: 0 OrderMaxNanFirst, 1 OrderMinNanLast, 2 OrderMaxNoNan,
// 3 OrderMinNanInf, 4 OrderMin.  b7dbg_argbest: one pass of the shared part kernel and the final kernel with the rows excl[0 .. n_excl)
// left out, n_excl <= 16: *row (-1: none) and *value.  b7dbg_argbest_loop: n <= 16 successive picks in one launch (above)
int b7dbg_argbest(b7_ctx *c, int order, const double *values, int64_t M, const long long *excl, int n_excl, double *value, long long *row) {
  return dbg_argbest_run(c, order, values, M, excl, n_excl, false, value, row);
}
int b7dbg_argbest_loop(b7_ctx *c, int order, const double *values, int64_t M, int n, double *values_out, long long *rows_out) {
  return dbg_argbest_run(c, order, values, M, nullptr, n, true, values_out, rows_out);
}
#endif

int b7_rff_compute(b7_ctx *c, const double *X, int64_t M1, int d, const double *omega, const double *phase, const double *W, int F, int q,
                   double *out) {
  if (!c) return B7_ERR_INVALID;
  if (!X || !omega || !phase || !W || !out) return b7_fail(c, B7_ERR_INVALID, "rff_compute: NULL argument");
  if (M1 < 1 || d < 1 || d > B7_MAX_D) return b7_fail(c, B7_ERR_INVALID, "rff_compute: M1 = %lld rows, d = %d (1..%d)", (long long)M1, d, B7_MAX_D);
  if (q < 1 || q > B7_BATCH_MAX) return b7_fail(c, B7_ERR_INVALID, "rff_compute: q = %d not in [1, %d]", q, B7_BATCH_MAX);
  if (F < 16 || F > B7_TS_MAX_FEATURES || F % 16)
    return b7_fail(c, B7_ERR_INVALID, "rff_compute: F = %d features: a multiple of 16 in [16, %d]", F, B7_TS_MAX_FEATURES);
  B7_HIP(c, hipSetDevice(c->device));
  const int dpad = rff_dpad(d);
  // X M1 d | out M1 q | omega F d | phase F | W F q | omf F dpad | wf 16 F -- a buffer of its own: the last nomination's paths and draws stay
  const size_t need = (size_t)M1 * d + (size_t)M1 * q + (size_t)F * d + F + (size_t)F * q + (size_t)F * dpad + 16 * (size_t)F;
  B7_TRY(b7_ensure(c, c->ts_user, sizeof(double) * need));
  double *Xd = (double *)c->ts_user.p, *od = Xd + (size_t)M1 * d, *omd = od + (size_t)M1 * q, *phd = omd + (size_t)F * d, *Wd = phd + F;
  double *omf = Wd + (size_t)F * q, *wf = omf + (size_t)F * dpad;
  B7_HIP(c, hipMemcpyAsync(Xd, X, sizeof(double) * (size_t)M1 * d, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(omd, omega, sizeof(double) * (size_t)F * d, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(phd, phase, sizeof(double) * F, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(Wd, W, sizeof(double) * (size_t)F * q, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_rff_pack(c, omd, F, d, Wd, q, 0, 1, q, 1.0, omf, wf));
  B7_TRY(launch_rff(c, Xd, M1, d, omf, phd, wf, F, nullptr, 0, od, q, 0, 1, q));
  B7_HIP(c, hipMemcpyAsync(out, od, sizeof(double) * (size_t)M1 * q, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays are consumed
  return B7_OK;
}

}  // extern "C"

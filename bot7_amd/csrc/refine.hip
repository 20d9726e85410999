// Off-grid refinement of a nomination: gradient ascent on the marginalised acquisition from the best grid rows.
//
// No counterpart in this reference's bots (bots/abstract.lua:118 nominates a grid row); Spearmint, which the reference descends
// from, hands its best grid rows to a local optimiser.  After b7_eval_nominate everything but the gradients is on the device: the
// S fits (BelKeep), the marginalised score over the grid, an arg-max that can leave rows out.  This file adds the posterior's
// gradient at 64 query columns per launch set and the loop that uses it; the score's gradient and the ladder are score.hip's
// (grad<K>, refine_step_kernel).
//
// With D_i = sum_c (x_c - X_ic)^2 w_c (w = 1 / lenscale_sq), k_i = k(x, X_i) and the radial factor g_i, dk_i/dx_c = -g_i (x_c - X_ic) w_c
// (ARD-SE: g = k; Matern-5/2: g = (5/3) amp (1 + s) exp(-s), s = sqrt(5 D)), V = inv(L) k*, W = inv(L)' V:
//   mu      = m + k* . alpha                     sigma^2      = amp - |V|^2           (the grid's L^-1 form)
//   dmu_c   = Ga_c - x_c w_c sum_i alpha_i g_i    dsigma^2_c  = -2 (GW_c - x_c w_c sum_i W_i g_i)
//   Ga = (alpha o g)' zsc,  GW = (W o g)' zsc     (zsc = X o w, the pre-scaled observations of the fit)
// The unit of work is 64 query columns (16 starts x 4 ladder rungs; b7_gp_grad_at: 64 rows of the caller's) against one hyper
// sample = blockIdx.z.  Every dependency between workgroups is a launch boundary: no flags, no spins, no cooperative barrier.
//   refine_k_kernel<KERN>  block = 64 observations: k and g, observations as rows (kt[Npad][64], gt[Npad][64]; ARD-SE stores one),
//                          the MFMA distance product and argument of ksx_kernel ((c - xs/2) - zs/2) -> cov_grad_nonpos4<KERN>
//   refine_v_kernel        block I of L^-1: V[I] = sum_{J <= I} Linv[I][J] kt[J] on MFMA, L^-1 streamed through LDS, the block's
//                          per-column sum of squares as one partial
//   refine_w_kernel        block J: W[J] = sum_{I >= J} Linv[I][J]' V[I] on MFMA, then with W[J] in registers block J's share of
//                          everything that contracts over the observations: sum alpha k, sum alpha g, sum W g and the two
//                          64 x dpad products on MFMA; one partial per block
//   refine_gather_kernel   the partials summed in block order: mu, sigma^2, dmu, dsigma^2 per column and sample
// All sums have one order, so the same call gives the same bits.  L^-1 is read once per product, sample and iteration.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"
#include "gemm_f64.h"
#include "ksx_exp.h"

namespace {

constexpr int RQ = 64;   // query columns of a launch set
constexpr int RB = 64;   // observations per block
constexpr int RLS = 65;  // LDS row stride of a staged 64 x 64 block of L^-1 (odd: conflict-free fragment reads)

// ---- A: k and g of 64 query columns against block blockIdx.x of the observations --------------------------------------------
// wave = one 16-column tile; A operand = the scaled observations (row = observation), B operand = the raw queries (column =
// query), so a lane's four results are four observations of one query and the stores run along the queries
template <int KERN>
__global__ void __launch_bounds__(256) refine_k_kernel(const double *__restrict__ xq, int d, int dpad, int Npad, int N,
                                                       const double *__restrict__ w_, const double *__restrict__ zsc_,
                                                       const double *__restrict__ zss_, const double *__restrict__ par,
                                                       double *__restrict__ kt_, double *__restrict__ gt_) {
  __shared__ double stab[128];
  const int64_t s = blockIdx.z;
  const double *w = w_ + s * dpad, *zsc = zsc_ + s * (int64_t)Npad * dpad, *zss = zss_ + s * Npad;
  double *kt = kt_ + s * (int64_t)Npad * RQ, *gt = gt_ ? gt_ + s * (int64_t)Npad * RQ : nullptr;
  const double amp = par[2 * s];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  if (tid < 128) stab[tid] = amp * b7_exp2_tab_dev[tid];
  const int q = wave * 16 + lr;  // this lane's query column
  double hq = 0.0;               // xs/2 in ascending k, as the grid's kernels form it
  for (int k = 0; k < d; ++k) {
    const double x = xq[q * d + k];
    hq = hq + (x * x) * w[k];
  }
  hq = 0.5 * hq;
  __syncthreads();
  const int ob0 = blockIdx.x * RB;
  const int ksteps = dpad >> 2;
  for (int t = 0; t < 4; ++t) {
    const double *orow = zsc + (int64_t)(ob0 + t * 16 + lr) * dpad + lq;
    d4_t c = {0.0, 0.0, 0.0, 0.0};
    for (int k4 = 0; k4 < ksteps; ++k4) {
      const int k = 4 * k4 + lq;
      const double a = orow[4 * k4];
      const double b = (k < d) ? xq[q * d + k] : 0.0;
      c = mfma_f64(a, b, c);
    }
    double arg[4], kv[4], gv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ob = ob0 + t * 16 + lq + 4 * r;
      arg[r] = (c[r] - hq) - ((ob < N) ? zss[ob] : 0.0);
    }
    cov_grad_nonpos4<KERN>(arg, stab, kv, gv);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ob = ob0 + t * 16 + lq + 4 * r;
      kt[(int64_t)ob * RQ + q] = (ob < N) ? kv[r] : 0.0;  // padding observations give exactly 0
      if (KERN != B7_KERNEL_ARDSE) gt[(int64_t)ob * RQ + q] = (ob < N) ? gv[r] : 0.0;
    }
  }
}

// a 64 x 64 block of L^-1 (rows r0.., columns c0..) into LDS, 256 threads, rows coalesced
__device__ __forceinline__ void stage_block(double *sL, const double *__restrict__ Linv, int Npad, int r0, int c0) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int idx = i * 256 + threadIdx.x, row = idx >> 6, col = idx & 63;
    sL[row * RLS + col] = Linv[(int64_t)(r0 + row) * Npad + c0 + col];
  }
}

// ---- B: V[I] = sum_{J <= I} Linv[I][J] kt[J]; blocks above the diagonal are never read ------------------------------------------
__global__ void __launch_bounds__(256) refine_v_kernel(const double *__restrict__ Linv_, int Npad, const double *__restrict__ kt_,
                                                       double *__restrict__ V_, double *__restrict__ vpart_) {
  __shared__ double sL[RB * RLS];
  const int64_t s = blockIdx.z;
  const int I = blockIdx.x, nb = gridDim.x;
  const double *Linv = Linv_ + s * (int64_t)Npad * Npad, *kt = kt_ + s * (int64_t)Npad * RQ;
  double *V = V_ + s * (int64_t)Npad * RQ, *vpart = vpart_ + (s * nb + I) * RQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const int col = wave * 16 + lr;
  d4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int J = 0; J <= I; ++J) {
    __syncthreads();
    stage_block(sL, Linv, Npad, I * RB, J * RB);
    __syncthreads();
    for (int k4 = 0; k4 < 16; ++k4) {
      const double b = kt[(int64_t)(J * RB + 4 * k4 + lq) * RQ + col];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma_f64(sL[(t * 16 + lr) * RLS + 4 * k4 + lq], b, acc[t]);
    }
  }
  double ss = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = acc[t][r];
      V[(int64_t)(I * RB + t * 16 + lq + 4 * r) * RQ + col] = v;
      ss = __builtin_fma(v, v, ss);
    }
  ss = ss + __shfl_xor(ss, 16);
  ss = ss + __shfl_xor(ss, 32);
  if (lq == 0) vpart[col] = ss;
}

// ---- C: W[J] = sum_{I >= J} Linv[I][J]' V[I], then block J's share of the contractions over the observations -----------------
// partial of (sample, J, column): sum alpha k | sum alpha g | sum W g | Ga[dpad] | GW[dpad]
__host__ __device__ constexpr int ref_pw(int dpad) { return 3 + 2 * dpad; }

__global__ void __launch_bounds__(256) refine_w_kernel(const double *__restrict__ Linv_, int Npad, int dpad,
                                                       const double *__restrict__ V_, const double *__restrict__ kt_,
                                                       const double *__restrict__ gt_, const double *__restrict__ alpha_,
                                                       const double *__restrict__ zsc_, double *__restrict__ cpart_) {
  __shared__ double sL[RB * RLS];
  const int64_t s = blockIdx.z;
  const int J = blockIdx.x, nb = gridDim.x, PW = ref_pw(dpad);
  const double *Linv = Linv_ + s * (int64_t)Npad * Npad, *V = V_ + s * (int64_t)Npad * RQ;
  const double *kt = kt_ + s * (int64_t)Npad * RQ, *gt = gt_ + s * (int64_t)Npad * RQ;
  const double *alpha = alpha_ + s * Npad, *zsc = zsc_ + s * (int64_t)Npad * dpad;
  double *cpart = cpart_ + (s * nb + J) * (int64_t)RQ * PW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const int col = wave * 16 + lr;
  d4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int I = J; I < nb; ++I) {
    __syncthreads();
    stage_block(sL, Linv, Npad, I * RB, J * RB);
    __syncthreads();
    for (int k4 = 0; k4 < 16; ++k4) {
      const double b = V[(int64_t)(I * RB + 4 * k4 + lq) * RQ + col];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma_f64(sL[(4 * k4 + lq) * RLS + t * 16 + lr], b, acc[t]);  // the block transposed
    }
  }
  // acc[t][r] = W[j][col], j = t 16 + lq + 4 r within the block
  double ag[4][4], wg[4][4], s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = J * RB + t * 16 + lq + 4 * r;
      const double kv = kt[(int64_t)j * RQ + col], gv = gt[(int64_t)j * RQ + col], al = alpha[j];
      ag[t][r] = al * gv;
      wg[t][r] = acc[t][r] * gv;
      s0 = __builtin_fma(al, kv, s0);
      s1 = s1 + ag[t][r];
      s2 = s2 + wg[t][r];
    }
  s0 = s0 + __shfl_xor(s0, 16), s1 = s1 + __shfl_xor(s1, 16), s2 = s2 + __shfl_xor(s2, 16);
  s0 = s0 + __shfl_xor(s0, 32), s1 = s1 + __shfl_xor(s1, 32), s2 = s2 + __shfl_xor(s2, 32);
  if (lq == 0) {
    double *o = cpart + (int64_t)col * PW;
    o[0] = s0, o[1] = s1, o[2] = s2;
  }
  // the two 64 x dpad products: A = (alpha o g)' and (W o g)' straight from the registers -- an MFMA's k slots may stand for any four
  // observations as long as both operands agree: slot lq of step (t, r) is observation t 16 + 4 r + lq --, B = zsc[J]
  for (int ct = 0; ct * 16 < dpad; ++ct) {
    const int cc = ct * 16 + lr;
    d4_t ga = {0.0, 0.0, 0.0, 0.0}, gw = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double b = (cc < dpad) ? zsc[(int64_t)(J * RB + t * 16 + 4 * r + lq) * dpad + cc] : 0.0;
        ga = mfma_f64(ag[t][r], b, ga);
        gw = mfma_f64(wg[t][r], b, gw);
      }
    if (cc < dpad) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double *o = cpart + (int64_t)(wave * 16 + lq + 4 * r) * PW + 3;
        o[cc] = ga[r];
        o[dpad + cc] = gw[r];
      }
    }
  }
}

// ---- the partials in block order: mu, sigma^2 and their gradients per column and sample.  1024 threads = 64 columns x 16 -------
__global__ void __launch_bounds__(1024) refine_gather_kernel(const double *__restrict__ cpart_, const double *__restrict__ vpart_,
                                                             int nb, int d, int dpad, const double *__restrict__ xq,
                                                             const double *__restrict__ w_, const double *__restrict__ par,
                                                             double *__restrict__ mu, double *__restrict__ var,
                                                             double *__restrict__ dmu, double *__restrict__ dvar) {
  const int64_t s = blockIdx.x;
  const int col = threadIdx.x >> 4, sub = threadIdx.x & 15, PW = ref_pw(dpad);
  const double *cpart = cpart_ + s * nb * (int64_t)RQ * PW + (int64_t)col * PW, *vpart = vpart_ + s * nb * RQ + col;
  const double *w = w_ + s * dpad;
  const double amp = par[2 * s], mean = par[2 * s + 1];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, vv = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double *o = cpart + (int64_t)b * RQ * PW;
    s0 = s0 + o[0], s1 = s1 + o[1], s2 = s2 + o[2];
    vv = vv + vpart[b * RQ];
  }
  if (sub == 0) {
    mu[s * RQ + col] = mean + s0;
    var[s * RQ + col] = amp - vv;
  }
  for (int c = sub; c < d; c += 16) {
    double ga = 0.0, gw = 0.0;
    for (int b = 0; b < nb; ++b) {
      const double *o = cpart + (int64_t)b * RQ * PW + 3;
      ga = ga + o[c];
      gw = gw + o[dpad + c];
    }
    const double xw = xq[col * d + c] * w[c];
    dmu[(s * RQ + col) * d + c] = ga - xw * s1;
    dvar[(s * RQ + col) * d + c] = -2.0 * (gw - xw * s2);
  }
}

// ---- the starts: TH's max over the accumulator, P times, the earlier winners left out ------------------------------------------
// (argbest.h: OrderMaxNanFirst over acc[row], start p leaving out the rows idx[0 .. p))

// the state of a call before iteration 0: start p at its grid row, and the 64 query rows (every rung at the start itself)
__global__ void __launch_bounds__(256) refine_init_kernel(RefState *__restrict__ st, const double *__restrict__ grid,
                                                          const double *__restrict__ acc, int d, int P, double eta0,
                                                          double *__restrict__ xq) {
  for (int e = threadIdx.x; e < B7_REFINE_MAX_STARTS * B7_MAX_D; e += blockDim.x) {
    const int p = e / B7_MAX_D, c = e % B7_MAX_D;
    const long long row = st->idx[p < P ? p : 0];
    const double x = (c < d) ? grid[row * d + c] : 0.0;
    st->x[p][c] = x;
    st->g[p][c] = 0.0;
    if (c < d)
      for (int k = 0; k < 4; ++k) xq[(p * 4 + k) * d + c] = x;
  }
  if (threadIdx.x < B7_REFINE_MAX_STARTS) {
    const int p = threadIdx.x;
    const double sc = acc[st->idx[p < P ? p : 0]];
    st->score[p] = sc;
    st->v[p] = NAN;
    st->eta[p] = eta0;
    st->status[p] = (p < P && sc == sc) ? 0 : B7_REFINE_NOT_RUN;
    st->active[p] = 0;
    if (p >= P) st->idx[p] = st->idx[0];
  }
}

// the workspace of 64 query columns against S fits, carved out of c->refine_ws
struct RefWork {
  double *xq[2];               // [64][d], ping-pong
  double *par;                 // [S][2] amp, mean
  double *box;                 // lo[d] | hi[d]
  double *kt, *gt, *V;         // [S][Npad][64]
  double *vpart, *cpart;       // [S][nb][64], [S][nb][64][PW]
  double *mu, *var, *dmu, *dvar;  // [S][64], [S][64][d]
  RefState *st;
  ArgBest *part;               // the top-P partials
};

int ref_work(b7_ctx *c, int S, int nparts, RefWork *wk) {
  const size_t n = (size_t)c->Npad, nb = n / RB, d = (size_t)c->dfit, PW = (size_t)ref_pw(c->dpad);
  size_t off = 0;
  auto take = [&](size_t doubles) {
    const size_t o = off;
    off += (doubles + 31) / 32 * 32;
    return o;
  };
  const size_t o_xq0 = take(RQ * d), o_xq1 = take(RQ * d), o_par = take(2 * (size_t)S), o_box = take(2 * d);
  const size_t o_kt = take(S * n * RQ), o_gt = take(S * n * RQ), o_V = take(S * n * RQ);
  const size_t o_vp = take(S * nb * RQ), o_cp = take(S * nb * RQ * PW);
  const size_t o_mu = take((size_t)S * RQ), o_var = take((size_t)S * RQ), o_dmu = take(S * RQ * d), o_dvar = take(S * RQ * d);
  const size_t o_st = take((sizeof(RefState) + 7) / 8), o_part = take(2 * (size_t)(nparts + 1));
  B7_TRY(b7_ensure(c, c->refine_ws, sizeof(double) * off));
  double *b = (double *)c->refine_ws.p;
  wk->xq[0] = b + o_xq0, wk->xq[1] = b + o_xq1, wk->par = b + o_par, wk->box = b + o_box;
  wk->kt = b + o_kt, wk->gt = b + o_gt, wk->V = b + o_V, wk->vpart = b + o_vp, wk->cpart = b + o_cp;
  wk->mu = b + o_mu, wk->var = b + o_var, wk->dmu = b + o_dmu, wk->dvar = b + o_dvar;
  wk->st = reinterpret_cast<RefState *>(b + o_st), wk->part = reinterpret_cast<ArgBest *>(b + o_part);
  return B7_OK;
}

// phases A-C and the gather for the 64 query rows in xq: mu, var, dmu, dvar of every sample of f into the workspace (the fits'
// amplitudes and means are read from wk.par)
int ref_posterior(b7_ctx *c, const FitSet &f, const RefWork &wk, const double *xq) {
  const int n = c->Npad, nb = n / RB, d = c->dfit, dpad = c->dpad, S = f.S;
  const bool se = c->kernel != B7_KERNEL_MATERN52;
  {
    PhaseScope ps(c, "refine:k");
    if (se)
      hipLaunchKernelGGL(refine_k_kernel<B7_KERNEL_ARDSE>, dim3(nb, 1, S), dim3(256), 0, c->stream, xq, d, dpad, n, c->N, f.w, f.zsc, f.zss,
                         (const double *)wk.par, wk.kt, (double *)nullptr);
    else
      hipLaunchKernelGGL(refine_k_kernel<B7_KERNEL_MATERN52>, dim3(nb, 1, S), dim3(256), 0, c->stream, xq, d, dpad, n, c->N, f.w, f.zsc,
                         f.zss, (const double *)wk.par, wk.kt, wk.gt);
  }
  {
    PhaseScope ps(c, "refine:v");
    hipLaunchKernelGGL(refine_v_kernel, dim3(nb, 1, S), dim3(256), 0, c->stream, f.Linv, n, (const double *)wk.kt, wk.V, wk.vpart);
  }
  {
    PhaseScope ps(c, "refine:w");
    hipLaunchKernelGGL(refine_w_kernel, dim3(nb, 1, S), dim3(256), 0, c->stream, f.Linv, n, dpad, (const double *)wk.V,
                       (const double *)wk.kt, (const double *)(se ? wk.kt : wk.gt), f.alpha, f.zsc, wk.cpart);
  }
  {
    PhaseScope ps(c, "refine:gather");
    hipLaunchKernelGGL(refine_gather_kernel, dim3(S), dim3(1024), 0, c->stream, (const double *)wk.cpart, (const double *)wk.vpart, nb,
                       d, dpad, xq, f.w, (const double *)wk.par, wk.mu, wk.var, wk.dmu, wk.dvar);
  }
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int refine_refuse(b7_ctx *c, const char *who, const b7_score_spec *spec) {
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: a communicator of %d ranks (refinement over a sharded grid is not built)", who, c->comm_world);
  if (spec && spec->kind == B7_SCORE_MES)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: max-value entropy search has no gradient piece (EI, LogEI and CB are built)", who);
  if (spec && spec->kind == B7_SCORE_LOGPI)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: log probability of improvement (LogPI) has no gradient piece (EI, LogEI and CB are built)", who);
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: %d response columns (one is built)", who, c->ycols);
  if (c->opts.var_with_noise || c->opts.var_clamp)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the gradient is the latent variance's (var_with_noise / var_clamp are set)", who);
  return B7_OK;
}

}  // namespace

extern "C" {

int b7_refine_default_opts(b7_refine_opts *out) {
  if (!out) return B7_ERR_INVALID;
  out->starts = 16, out->iters = 16, out->eta0 = 1.0 / 16.0, out->lo = nullptr, out->hi = nullptr;
  return B7_OK;
}

int b7_eval_nominate_refine(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, const b7_refine_opts *opts,
                            double *best_val, int64_t *best_idx1, double *x_out, double *val_out, int64_t *start_idx1_out,
                            double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "eval_nominate_refine: this context belongs to a group (sharded refinement is not built)");
  if (!opts || !best_val || !best_idx1 || !x_out || !val_out || !start_idx1_out)
    return b7_fail(c, B7_ERR_INVALID, "eval_nominate_refine: NULL argument (opts, best_val, best_idx1, x_out, val_out, start_idx1_out are required)");
  if (c->comm && c->comm_world > 1) return refine_refuse(c, "eval_nominate_refine", spec);
  B7_TRY(eval_validate(c, S, hyps, spec, 0));
  B7_TRY(refine_refuse(c, "eval_nominate_refine", spec));
  const int P = opts->starts, iters = opts->iters, d = c->dfit;
  if (P < 1 || P > B7_REFINE_MAX_STARTS || P > c->M)
    return b7_fail(c, B7_ERR_INVALID, "eval_nominate_refine: starts = %d not in [1, %d], or above the grid's %lld rows", P, B7_REFINE_MAX_STARTS, (long long)c->M);
  if (iters < 0 || iters > B7_REFINE_MAX_ITERS) return b7_fail(c, B7_ERR_INVALID, "eval_nominate_refine: iters = %d not in [0, %d]", iters, B7_REFINE_MAX_ITERS);
  if (!(opts->eta0 > 0.0 && opts->eta0 <= 1.0)) return b7_fail(c, B7_ERR_INVALID, "eval_nominate_refine: eta0 = %g not in (0, 1]", opts->eta0);
  if ((opts->lo == nullptr) != (opts->hi == nullptr)) return b7_fail(c, B7_ERR_INVALID, "eval_nominate_refine: lo and hi go together");
  std::vector<double> box(2 * (size_t)d);
  for (int k = 0; k < d; ++k) {
    box[k] = opts->lo ? opts->lo[k] : 0.0, box[d + k] = opts->hi ? opts->hi[k] : 1.0;
    if (!std::isfinite(box[k]) || !std::isfinite(box[d + k]) || !(box[k] < box[d + k]))
      return b7_fail(c, B7_ERR_INVALID, "eval_nominate_refine: box column %d is [%g, %g] (finite, lo < hi)", k, box[k], box[d + k]);
  }
  B7_HIP(c, hipSetDevice(c->device));
  c->refine_valid = false;
  std::vector<double> jit(S, 0.0);
  if (jitter_out) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out) std::fill(info_out, info_out + S, 0);
  // b7_eval_nominate's own protocol and launches; the S fits are kept on the way (no copy of the means and variances)
  BelKeep keep;
  keep.want_alpha = true;
  B7_TRY(nominate_run(
      c, "eval_nominate_refine", B7_OK, 0, (double)S, [&](ScoreParams *pend) { return eval_enqueue(c, S, hyps, spec, pend, &keep); },
      [&]() { return reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, true); },
      [&]() { return eval_redo(c, S, hyps, spec, jit.data(), info_out, &keep); }, best_val, best_idx1));
  if (jitter_out) memcpy(jitter_out, jit.data(), sizeof(double) * S);
  c->fitted = false;  // the context's own fit slot holds none of the samples, as after b7_eval_nominate
  c->predicted = false;
  if (*best_idx1 < 1 || *best_idx1 > c->M) return b7_fail(c, B7_ERR_STATE, "eval_nominate_refine: the nomination named no row");

  const int nparts = (int)std::min<int64_t>((c->M + 255) / 256, (int64_t)c->cus * 8);
  RefWork wk;
  B7_TRY(ref_work(c, S, nparts, &wk));
  std::vector<double> par(2 * (size_t)S);
  for (int s = 0; s < S; ++s) par[2 * s] = hyps[s].amp, par[2 * s + 1] = hyps[s].mean;
  B7_HIP(c, hipMemcpyAsync(wk.par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(wk.box, box.data(), sizeof(double) * box.size(), hipMemcpyHostToDevice, c->stream));
  const long long first = *best_idx1 - 1;
  B7_HIP(c, hipMemcpyAsync(&wk.st->idx[0], &first, sizeof(long long), hipMemcpyHostToDevice, c->stream));
  const double *acc = (const double *)c->acc.p, *grid = (const double *)c->grid[c->grid_cur].p;
  {
    PhaseScope ps(c, "refine:starts");
    for (int p = 1; p < P; ++p) {
      launch_argbest<OrderMaxNanFirst>(c->stream, ArgLoadStrided{acc, 1}, (long long)c->M, nparts, wk.part, p, wk.st->idx, (double *)nullptr);
    }
    hipLaunchKernelGGL(refine_init_kernel, dim3(1), dim3(256), 0, c->stream, wk.st, grid, acc, d, P, opts->eta0, wk.xq[0]);
    B7_HIP(c, hipGetLastError());
  }
  double *trace = nullptr;
  c->refine_trace_P = 0;
  if (c->refine_trace_on) {
    const size_t tb = sizeof(double) * (size_t)P * (iters + 1) * B7_REFINE_TRACE_WIDTH;
    B7_TRY(b7_ensure(c, c->refine_trace, tb));
    B7_HIP(c, hipMemsetAsync(c->refine_trace.p, 0, tb, c->stream));
    trace = (double *)c->refine_trace.p;
  }
  double *fd = nullptr;
  if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
  ScoreParams sp = score_params(c, spec, fd);
  sp.S = S;
  for (int it = 0; it <= iters; ++it) {
    const double *xq = wk.xq[it & 1];
    B7_TRY(ref_posterior(c, keep.fits, wk, xq));
    RefStep rs;
    rs.mu = wk.mu, rs.var = wk.var, rs.dmu = wk.dmu, rs.dvar = wk.dvar;
    rs.xq = xq, rs.xq_next = wk.xq[(it + 1) & 1], rs.st = wk.st, rs.trace = trace;
    rs.lo = wk.box, rs.hi = wk.box + d;
    rs.d = d, rs.P = P, rs.iter = it, rs.iters = iters, rs.eta0 = opts->eta0;
    B7_TRY(launch_refine_step(c, sp, rs));
  }
  RefState hs;
  B7_HIP(c, hipMemcpyAsync(&hs, wk.st, sizeof(RefState), hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  // the winner: the highest final value among the starts that ran, the lowest start order on ties; if none moved, the nominee
  int win = 0;
  bool moved = false;
  for (int p = 0; p < P; ++p) moved = moved || (hs.status[p] & B7_REFINE_MOVED);
  if (moved) {
    int best = -1;
    for (int p = 0; p < P; ++p) {
      if ((hs.status[p] & B7_REFINE_NOT_RUN) || !std::isfinite(hs.v[p])) continue;
      if (best < 0 || hs.v[p] > hs.v[best]) best = p;
    }
    if (best >= 0) win = best;
  }
  memcpy(x_out, hs.x[win], sizeof(double) * d);
  *val_out = hs.v[win];
  *start_idx1_out = hs.idx[win] + 1;
  c->refine_P = P, c->refine_d = d, c->refine_iters = iters;
  c->refine_last = hs;
  c->refine_valid = true;
  if (trace) c->refine_trace_P = P, c->refine_trace_iters = iters;
  return B7_OK;
}

int b7_refine_last(b7_ctx *c, int *P, double *x, double *val, int64_t *start_idx1, int *status) {
  if (!c) return B7_ERR_INVALID;
  if (!c->refine_valid) return b7_fail(c, B7_ERR_STATE, "refine_last: no successful b7_eval_nominate_refine on this context");
  const RefState &hs = c->refine_last;
  if (P) *P = c->refine_P;
  for (int p = 0; p < c->refine_P; ++p) {
    if (x) memcpy(x + (size_t)p * c->refine_d, hs.x[p], sizeof(double) * c->refine_d);
    if (val) val[p] = hs.v[p];
    if (start_idx1) start_idx1[p] = hs.idx[p] + 1;
    if (status) status[p] = hs.status[p];
  }
  return B7_OK;
}

int b7_refine_shape(b7_ctx *c, int *P, int *d, int *iters, int *traced) {
  if (!c) return B7_ERR_INVALID;
  if (!c->refine_valid) return b7_fail(c, B7_ERR_STATE, "refine_shape: no successful b7_eval_nominate_refine on this context");
  if (P) *P = c->refine_P;
  if (d) *d = c->refine_d;
  if (iters) *iters = c->refine_iters;
  if (traced) *traced = c->refine_trace_P > 0 ? 1 : 0;
  return B7_OK;
}

int b7_refine_trace_enable(b7_ctx *c, int on) {
  if (!c) return B7_ERR_INVALID;
  c->refine_trace_on = on != 0;
  c->refine_trace_P = 0;
  return B7_OK;
}

int b7_refine_trace(b7_ctx *c, int start, double *records, int *n_records) {
  if (!c) return B7_ERR_INVALID;
  if (!n_records) return b7_fail(c, B7_ERR_INVALID, "refine_trace: NULL argument");
  if (!c->refine_valid || c->refine_trace_P < 1)
    return b7_fail(c, B7_ERR_STATE, "refine_trace: no traced b7_eval_nominate_refine (b7_refine_trace_enable first)");
  if (start < 0 || start >= c->refine_trace_P) return b7_fail(c, B7_ERR_INVALID, "refine_trace: start %d of %d", start, c->refine_trace_P);
  B7_HIP(c, hipSetDevice(c->device));
  const size_t per = (size_t)(c->refine_trace_iters + 1) * B7_REFINE_TRACE_WIDTH;
  if (records)
    B7_HIP(c, hipMemcpy(records, (const double *)c->refine_trace.p + per * start, sizeof(double) * per, hipMemcpyDeviceToHost));
  *n_records = c->refine_trace_iters + 1;
  return B7_OK;
}

int b7_gp_grad_at(b7_ctx *c, const double *X1, int64_t M1, double *mean, double *var, double *dmean, double *dvar) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted || c->model_kind != 0) return b7_fail(c, B7_ERR_STATE, "gp_grad_at: no GP fit on this context");
  if (M1 < 0 || (!X1 && M1 > 0)) return b7_fail(c, B7_ERR_INVALID, "gp_grad_at: bad X1/M1");
  B7_TRY(refine_refuse(c, "gp_grad_at", nullptr));
  if (M1 == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const int d = c->dfit;
  RefWork wk;
  B7_TRY(ref_work(c, 1, 1, &wk));
  const FitSet fit = ctx_fit(c);
  const double par[2] = {fit.amp, fit.mean};
  B7_HIP(c, hipMemcpyAsync(wk.par, par, sizeof(par), hipMemcpyHostToDevice, c->stream));
  std::vector<double> chunk((size_t)RQ * d);
  for (int64_t r0 = 0; r0 < M1; r0 += RQ) {
    const int rows = (int)std::min<int64_t>(RQ, M1 - r0);
    for (int r = 0; r < RQ; ++r)  // a short chunk repeats its last row
      memcpy(&chunk[(size_t)r * d], X1 + (size_t)(r0 + std::min(r, rows - 1)) * d, sizeof(double) * d);
    B7_HIP(c, hipMemcpyAsync(wk.xq[0], chunk.data(), sizeof(double) * chunk.size(), hipMemcpyHostToDevice, c->stream));
    B7_TRY(ref_posterior(c, fit, wk, wk.xq[0]));
    if (mean) B7_HIP(c, hipMemcpyAsync(mean + r0, wk.mu, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    if (var) B7_HIP(c, hipMemcpyAsync(var + r0, wk.var, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    if (dmean) B7_HIP(c, hipMemcpyAsync(dmean + (size_t)r0 * d, wk.dmu, sizeof(double) * rows * d, hipMemcpyDeviceToHost, c->stream));
    if (dvar) B7_HIP(c, hipMemcpyAsync(dvar + (size_t)r0 * d, wk.dvar, sizeof(double) * rows * d, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));  // the staging chunk is free again
  }
  return B7_OK;
}

int b7_score_grad_compute(b7_ctx *c, const b7_score_spec *spec, int S, const double *mean, const double *var, const double *dmean,
                          const double *dvar, int64_t M1, int d, double *value, double *grad) {
  if (!c) return B7_ERR_INVALID;
  if (!spec || S < 1 || M1 < 0 || d < 1 || d > B7_MAX_D || (M1 > 0 && (!mean || !var || !dmean || !dvar || !value || !grad)))
    return b7_fail(c, B7_ERR_INVALID, "score_grad_compute: bad arguments");
  if (spec->kind == B7_SCORE_MES) return b7_fail(c, B7_ERR_UNSUPPORTED, "score_grad_compute: max-value entropy search has no gradient piece");
  if (spec->kind == B7_SCORE_LOGPI)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "score_grad_compute: log probability of improvement (LogPI) has no gradient piece");
  if (spec->kind != B7_SCORE_EI && spec->kind != B7_SCORE_CB && spec->kind != B7_SCORE_LOGEI)
    return b7_fail(c, B7_ERR_INVALID, "score_grad_compute: unknown score kind %d", spec->kind);
  if (score_needs_fmin(spec->kind) && !spec->fmin) return b7_fail(c, B7_ERR_INVALID, "score_grad_compute: EI needs fmin");
  if (M1 == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t SM = (size_t)S * M1, SMd = SM * d;
  B7_TRY(b7_ensure(c, c->refine_user, sizeof(double) * (2 * SM + 2 * SMd + (size_t)M1 * (d + 1))));
  double *b = (double *)c->refine_user.p, *mu_d = b, *var_d = b + SM, *dmu_d = var_d + SM, *dvar_d = dmu_d + SMd, *val_d = dvar_d + SMd,
         *grad_d = val_d + M1;
  B7_HIP(c, hipMemcpyAsync(mu_d, mean, sizeof(double) * SM, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(var_d, var, sizeof(double) * SM, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(dmu_d, dmean, sizeof(double) * SMd, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(dvar_d, dvar, sizeof(double) * SMd, hipMemcpyHostToDevice, c->stream));
  ScoreParams sp;
  sp.kind = spec->kind, sp.upper = spec->upper, sp.tradeoff = spec->tradeoff, sp.sign = spec->sign;
  sp.fmin = nullptr, sp.fmin0 = score_needs_fmin(spec->kind) ? spec->fmin[0] : 0.0;
  sp.S = S;
  B7_TRY(launch_score_grad(c, sp, mu_d, var_d, dmu_d, dvar_d, M1, d, val_d, grad_d));
  B7_HIP(c, hipMemcpyAsync(value, val_d, sizeof(double) * M1, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(grad, grad_d, sizeof(double) * (size_t)M1 * d, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

}  // extern "C"

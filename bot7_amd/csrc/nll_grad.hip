// The gradient of the negative log marginal likelihood of a finished GP fit, and the bounded fit that descends on it.
//
// No counterpart in this reference: its only way to hypers is the slice sampler (samplers/slice.lua).  In the sampler's own
// coordinates theta = [log lenscale_sq_1 .. log lenscale_sq_d, log amp, log noise, mean], with Q = inv(K) - alpha alpha',
// Kf = K - noise I, D_ij = sum_k (x_ik - x_jk)^2 w_k (w = 1 / lenscale_sq) and the radial factor g (dk/dD = -g/2: ARD-SE g = k,
// Matern-5/2 g = (5/3) amp (1 + s) exp(-s), ksx_exp.h cov_grad_nonpos4):
//   d nll / d log lenscale_sq_k = 1/4 sum_ij Q_ij g_ij (x_ik - x_jk)^2 w_k      (dK_ij / d log lenscale_sq_k = g_ij/2 (x_ik - x_jk)^2 w_k)
//   d nll / d log amp            = 1/2 sum_ij Q_ij Kf_ij
//   d nll / d log noise          = 1/2 noise (sum_ij Linv_ij^2 - sum_i alpha_i^2)  (tr inv(K) = |Linv|_F^2; exactly 0 at noise == 0)
//   d nll / d mean               = -sum_i alpha_i
// from d nll = 1/2 tr(Q dK) - alpha' d(mean) 1.  A jitter the schedule added sits in Linv and alpha as a constant on the diagonal.
//
// nll_grad_kernel<KERN>: one workgroup owns the 64 x 64 tile (I, J), I >= J, of Q.  It accumulates inv(K)_IJ = sum_{r >= 64 I}
// Linv[r][I]' Linv[r][J] over the rows below it on v_mfma_f64_16x16x4 (32-row stages of the two column blocks through LDS, the
// next stage's loads in flight during the MFMAs), and with the tile still in its accumulator registers subtracts alpha_i alpha_j,
// forms k_ij and g_ij as refine_k_kernel does (the MFMA distance product of the scaled observations with the raw ones, the
// argument (c - xs/2) - zs/2, cov_grad_nonpos4<KERN>) and contracts: d sums of Q g (x_ik - x_jk)^2 on the raw observations, the sum
// of Q k, and on diagonal tiles the trace of inv(K).  inv(K) is never stored.  Off-diagonal tiles count twice.  Rows and columns
// >= N are masked to exactly 0, and rows of Linv >= N are never multiplied in, whatever the padding holds.
// Tile t = I (I + 1) / 2 + J is blockIdx.x: the tiles of small I, whose chains are the longest, start first.
// nll_grad_fold_kernel: the second launch; the partials [tile][d + 2] summed per component in one fixed order, the alpha terms, the
// factors.  The launch boundary is the only dependency between the two; every sum has one order, whatever runs side by side.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include <vector>

#include "b7_internal.h"
#include "gemm_f64.h"
#include "ksx_exp.h"
#include "lbfgsb.h"

namespace {

constexpr int GT = 64;    // tile edge
constexpr int GK = 32;    // rows of L^-1 per stage
constexpr int GLS = 80;   // LDS row stride of a stage (doubles): the four k-rows of a fragment read land in disjoint bank halves
constexpr int GXS = 33;   // LDS row stride of a 64 x 32 chunk of raw observations
constexpr int GC = 32;    // input dimensions per chunk of the lengthscale contraction

__device__ __forceinline__ double wave_sum(double v) {  // one fixed butterfly: the same bits on every run
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

template <int KERN>
__global__ void __launch_bounds__(256) nll_grad_kernel(const double *__restrict__ Linv, const double *__restrict__ alpha,
                                                       const double *__restrict__ w, const double *__restrict__ zsc,
                                                       const double *__restrict__ zss, const double *__restrict__ xobs, int N, int Npad,
                                                       int d, int dpad, double amp, double *__restrict__ part) {
  __shared__ __align__(16) double sm[2 * GK * GLS];   // a stage of the two column blocks; afterwards the raw observations' chunks
  __shared__ double stab[128];
  __shared__ double wsum[4][B7_MAX_D + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  // tile (I, J) of blockIdx.x = I (I + 1) / 2 + J
  const int t = blockIdx.x;
  int I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int i0 = I * GT, j0 = J * GT;
  if (tid < 128) stab[tid] = amp * b7_exp2_tab_dev[tid];

  // ---- inv(K)_IJ on MFMA: A[m][k] = Linv[k][i0 + m], B[k][n] = Linv[k][j0 + n]
  d4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4_t{0.0, 0.0, 0.0, 0.0};
  double *sA = sm, *sB = sm + GK * GLS;
  const int kend = (N + GK - 1) / GK * GK;  // <= Npad: Npad is a multiple of 64
  d2_t ra[4], rb[4];
  auto load_stage = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256, row = idx >> 5, c2 = idx & 31;
      const int r = k0 + row;
      if (r < N) {
        ra[i] = *reinterpret_cast<const d2_t *>(Linv + (int64_t)r * Npad + i0 + 2 * c2);
        rb[i] = *reinterpret_cast<const d2_t *>(Linv + (int64_t)r * Npad + j0 + 2 * c2);
      } else {
        ra[i] = d2_t{0.0, 0.0};
        rb[i] = d2_t{0.0, 0.0};
      }
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256, row = idx >> 5, c2 = idx & 31;
      *reinterpret_cast<d2_t *>(sA + row * GLS + 2 * c2) = ra[i];
      *reinterpret_cast<d2_t *>(sB + row * GLS + 2 * c2) = rb[i];
    }
  };
  load_stage(i0);
  for (int k0 = i0; k0 < kend; k0 += GK) {
    __syncthreads();  // the previous stage has been read
    store_stage();
    __syncthreads();
    if (k0 + GK < kend) load_stage(k0 + GK);
    const double *pa = sA + lq * GLS + wm * 32 + lr, *pb = sB + lq * GLS + wn * 32 + lr;
#pragma unroll
    for (int s = 0; s < GK / 4; ++s) {
      const double a0 = pa[4 * s * GLS], a1 = pa[4 * s * GLS + 16];
      const double b0 = pb[4 * s * GLS], b1 = pb[4 * s * GLS + 16];
      acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
      acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
      acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
      acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
    }
  }

  // ---- epilogue in the accumulator registers: element (a, b, r) is row i0 + 32 wm + 16 a + lq + 4 r, column j0 + 32 wn + 16 b + lr
  const int ibase = i0 + wm * 32, jbase = j0 + wn * 32;
  double hq[2], aj[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int j = jbase + 16 * b + lr;
    double h = 0.0;  // xs/2 in ascending k, as the grid's kernels form it
    if (j < N)
      for (int k = 0; k < d; ++k) {
        const double x = xobs[(int64_t)j * d + k];
        h = h + (x * x) * w[k];
      }
    hq[b] = 0.5 * h;
    aj[b] = alpha[j];
  }
  double qg[2][2][4];
  double sk = 0.0, tr = 0.0;
  const int ksteps = dpad >> 2;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const double *orow = zsc + (int64_t)(ibase + 16 * a + lr) * dpad + lq;
      const int jc = jbase + 16 * b + lr;
      d4_t c = {0.0, 0.0, 0.0, 0.0};
      for (int k4 = 0; k4 < ksteps; ++k4) {
        const int k = 4 * k4 + lq;
        const double av = orow[4 * k4];
        const double bv = (k < d && jc < N) ? xobs[(int64_t)jc * d + k] : 0.0;
        c = mfma_f64(av, bv, c);
      }
      double arg[4], kv[4], gv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ibase + 16 * a + lq + 4 * r;
        arg[r] = (c[r] - hq[b]) - ((i < N) ? zss[i] : 0.0);
      }
      cov_grad_nonpos4<KERN>(arg, stab, kv, gv);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ibase + 16 * a + lq + 4 * r;
        const bool live = i < N && jc < N;
        const double kinv = acc[a][b][r];
        const double q = live ? kinv - alpha[i] * aj[b] : 0.0;
        sk = sk + (live ? q * kv[r] : 0.0);
        qg[a][b][r] = live ? q * gv[r] : 0.0;
        if (live && i == jc) tr = tr + kinv;
      }
    }
  }
  {
    const double s1 = wave_sum(sk), s2 = wave_sum(tr);
    if (lane == 0) wsum[wave][d] = s1, wsum[wave][d + 1] = s2;
  }
  // the lengthscale sums on the raw observations, GC dimensions at a time through LDS (the stage buffer is free now)
  double *xI = sm, *xJ = sm + GT * GXS;
  for (int kc = 0; kc < d; kc += GC) {
    const int nk = d - kc < GC ? d - kc : GC;
    __syncthreads();
    for (int e = tid; e < GT * GC; e += 256) {
      const int row = e >> 5, k = e & 31;
      const bool in = k < nk;
      xI[row * GXS + k] = (in && i0 + row < N) ? xobs[(int64_t)(i0 + row) * d + kc + k] : 0.0;
      xJ[row * GXS + k] = (in && j0 + row < N) ? xobs[(int64_t)(j0 + row) * d + kc + k] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      double s = 0.0;
      const double xj0 = xJ[(wn * 32 + lr) * GXS + k], xj1 = xJ[(wn * 32 + 16 + lr) * GXS + k];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double xi = xI[(wm * 32 + 16 * a + lq + 4 * r) * GXS + k];
          const double d0 = xi - xj0, d1 = xi - xj1;
          s = s + qg[a][0][r] * (d0 * d0);
          s = s + qg[a][1][r] * (d1 * d1);
        }
      s = wave_sum(s);
      if (lane == 0) wsum[wave][kc + k] = s;
    }
  }
  __syncthreads();
  if (tid < d + 2) {
    double v = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
    if (I != J && tid <= d) v = 2.0 * v;  // the mirror tile; the trace lives on diagonal tiles alone
    part[(int64_t)t * (d + 2) + tid] = v;
  }
}

// component c = blockIdx.x of the gradient: c < d + 2 folds the tiles' partials (thread t takes tiles t, t + 256, .. in ascending
// order, then the 256 sums in a fixed tree); the noise component (c == d + 1) and the mean (c == d + 2) also fold alpha
__global__ void __launch_bounds__(256) nll_grad_fold_kernel(const double *__restrict__ part, int ntiles, int d, const double *__restrict__ w,
                                                            const double *__restrict__ alpha, int N, double noise,
                                                            double *__restrict__ grad) {
  __shared__ double red[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  auto tree = [&](double v) {
    red[tid] = v;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (tid < h) red[tid] = red[tid] + red[tid + h];
      __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
  };
  double s = 0.0;
  if (c < d + 2)
    for (int t = tid; t < ntiles; t += 256) s = s + part[(int64_t)t * (d + 2) + c];
  const double tiles = tree(s);
  double a = 0.0;
  if (c >= d + 1)
    for (int i = tid; i < N; i += 256) a = a + (c == d + 1 ? alpha[i] * alpha[i] : alpha[i]);
  const double asum = tree(a);
  if (tid == 0) {
    double g;
    if (c < d) g = 0.25 * (tiles * w[c]);
    else if (c == d) g = 0.5 * tiles;
    else if (c == d + 1) g = noise == 0.0 ? 0.0 : 0.5 * noise * (tiles - asum);
    else g = -asum;
    grad[c] = g;
  }
}

// the partials' buffer of the context: [ntiles][d + 2] partials, then the d + 3 components
int grad_buf_ensure(b7_ctx *c, int *ntiles_out, double **grad_dev) {
  const int nbt = (c->N + GT - 1) / GT, ntiles = nbt * (nbt + 1) / 2, d = c->dfit;
  const size_t doubles = (size_t)ntiles * (d + 2) + (d + 3);
  B7_TRY(b7_ensure(c, c->gradpart, sizeof(double) * doubles));
  B7_TRY(b7_pin_ensure(c, c->pin_grad, sizeof(double) * (B7_MAX_D + 3), false));
  *ntiles_out = ntiles;
  *grad_dev = (double *)c->gradpart.p + (size_t)ntiles * (d + 2);
  return B7_OK;
}

}  // namespace

// The gradient of fit f of the context's data (raw observations xobs), d + 3 components into grad_dev: two launches on c's stream
int launch_nll_grad(b7_ctx *c, const FitSet &f, const double *xobs, double *part, int ntiles, double *grad_dev) {
  PhaseScope ps(c, "nll_grad");
  const int N = c->N, d = c->dfit;
  if (N < 1 || f.Npad < N || f.Npad % GT != 0 || d < 1 || d > B7_MAX_D || f.dpad < d || f.dpad % 4 != 0 || !f.Linv || !f.alpha || !xobs ||
      ntiles != ((N + GT - 1) / GT) * ((N + GT - 1) / GT + 1) / 2)
    return b7_fail(c, B7_ERR_INVALID, "nll_grad: N %d Npad %d d %d dpad %d outside the kernel's shapes", N, f.Npad, d, f.dpad);
  if (c->kernel == B7_KERNEL_MATERN52)
    hipLaunchKernelGGL(nll_grad_kernel<B7_KERNEL_MATERN52>, dim3(ntiles), dim3(256), 0, c->stream, f.Linv, f.alpha, f.w, f.zsc, f.zss, xobs,
                       N, f.Npad, d, f.dpad, f.amp, part);
  else
    hipLaunchKernelGGL(nll_grad_kernel<B7_KERNEL_ARDSE>, dim3(ntiles), dim3(256), 0, c->stream, f.Linv, f.alpha, f.w, f.zsc, f.zss, xobs, N,
                       f.Npad, d, f.dpad, f.amp, part);
  hipLaunchKernelGGL(nll_grad_fold_kernel, dim3(d + 3), dim3(256), 0, c->stream, (const double *)part, ntiles, d, f.w, f.alpha, N, f.noise,
                     grad_dev);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// fit_hyp_core's hook (c->grad_hook): the gradient of the fit just enqueued and its copy to pinned memory, behind the fit's tail and
// ahead of the one synchronisation that ends the fit.  The buffers were sized by the caller before anything was in flight.
int nll_grad_enqueue(b7_ctx *c) {
  int ntiles = 0;
  double *grad_dev = nullptr;
  B7_TRY(grad_buf_ensure(c, &ntiles, &grad_dev));
  B7_TRY(launch_nll_grad(c, ctx_fit(c), (const double *)c->xobs.p, (double *)c->gradpart.p, ntiles, grad_dev));
  B7_HIP(c, hipMemcpyAsync(c->pin_grad.host, grad_dev, sizeof(double) * (c->dfit + 3), hipMemcpyDeviceToHost, c->stream));
  return B7_OK;
}

namespace {

// what both gradient entry points refuse, by code and name
int grad_guard(b7_ctx *c, const char *who) {
  if (c->group) return b7_fail(c, B7_ERR_STATE, "%s: this context belongs to a group (likelihood gradients over sharded data are not built)", who);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: a communicator of %d ranks (likelihood gradients over sharded data are not built)", who,
                   c->comm_world);
  return B7_OK;
}

void grad_out_copy(const b7_ctx *c, double jitter, double *grad_out) {
  const int n = c->dfit + 3;
  if (jitter < 0.0)  // the chol(I) fallback: what the context holds is not a factor of K
    for (int k = 0; k < n; ++k) grad_out[k] = NAN;
  else
    memcpy(grad_out, c->pin_grad.host, sizeof(double) * n);
}

}  // namespace

extern "C" {

int b7_gp_fit_hyp_grad(b7_ctx *c, const b7_hyp *hyp, double *nll_out, double *grad_out, double *jitter_used, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(grad_guard(c, "gp_fit_hyp_grad"));
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "gp_fit_hyp_grad: call b7_gp_set_data first");
  if (!grad_out) return b7_fail(c, B7_ERR_INVALID, "gp_fit_hyp_grad: grad_out is NULL");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_fit_hyp_grad: %d response columns (the gradient of one column is built)", c->ycols);
  B7_TRY(check_hyp(c, hyp, c->dfit));
  B7_HIP(c, hipSetDevice(c->device));
  int ntiles = 0;
  double *grad_dev = nullptr;
  B7_TRY(grad_buf_ensure(c, &ntiles, &grad_dev));  // sized before anything is in flight
  double jitter = 0.0;
  c->grad_hook = true;
  const int rc = fit_hyp_core(c, hyp, nll_out, &jitter, info_out, false);
  c->grad_hook = false;
  B7_TRY(rc);
  if (jitter_used) *jitter_used = jitter;
  grad_out_copy(c, jitter, grad_out);
  return B7_OK;
}

int b7_gp_nll_grad(b7_ctx *c, double *grad_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(grad_guard(c, "gp_nll_grad"));
  if (!grad_out) return b7_fail(c, B7_ERR_INVALID, "gp_nll_grad: grad_out is NULL");
  if (c->fitted && c->model_kind == 1) return b7_fail(c, B7_ERR_STATE, "gp_nll_grad: the context's fit is a Bayesian-linear head's, not a GP's");
  if (c->fitted && !c->gfit && c->clf_mode_valid && c->clf_epoch == c->epoch)
    return b7_fail(c, B7_ERR_STATE, "gp_nll_grad: the context's fit is a classifier's Laplace fit (b7_clf_fit_hyp), not a GP regressor's");
  if (!c->fitted || !c->gfit || c->gfit_N != c->N)
    return b7_fail(c, B7_ERR_STATE, "gp_nll_grad: no GP fit of the resident data on this context (call b7_gp_fit_hyp first)");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_nll_grad: %d response columns (the gradient of one column is built)", c->ycols);
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(nll_grad_enqueue(c));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  grad_out_copy(c, c->gfit_jitter, grad_out);
  return B7_OK;
}

// ---- the bounded fit -----------------------------------------------------------------------------------------------------------

struct MapCall {
  b7_ctx *c;
  int d, rc;
  std::vector<double> ls, last;  // the lengthscales of the evaluation in flight; the point the context's fit slot was last fitted at
  bool last_ok;
};

static void map_hyp(MapCall *m, const double *theta, b7_hyp *h) {
  const int d = m->d;
  for (int k = 0; k < d; ++k) m->ls[k] = exp(theta[k]);
  h->lenscale_sq = m->ls.data(), h->amp = exp(theta[d]), h->noise = exp(theta[d + 1]), h->mean = theta[d + 2];
}

static int map_fn(void *user, int n, const double *theta, double *f, double *g) {
  MapCall *m = static_cast<MapCall *>(user);
  b7_hyp h;
  map_hyp(m, theta, &h);
  double nll = NAN, jitter = 0.0;
  int info = 0;
  m->last_ok = false;
  const int rc = b7_gp_fit_hyp_grad(m->c, &h, &nll, g, &jitter, &info);
  if (rc == B7_ERR_INVALID) {  // exp() left the hypers' domain (overflow, or underflow to 0): a failed trial point, not a failed call
    *f = NAN;
    return 0;
  }
  if (rc != B7_OK) {
    m->rc = rc;
    return 1;  // stop: the message is the fit's
  }
  memcpy(m->last.data(), theta, sizeof(double) * n);
  m->last_ok = true;
  *f = jitter < 0.0 ? NAN : nll;  // the chol(I) fallback is a failed trial point
  return 0;
}

int b7_gp_fit_map(b7_ctx *c, const double *theta0, const double *lo, const double *hi, const b7_lbfgsb_opts *opts, double *theta_out,
                  double *nll_out, double *grad_out, int *iters_out, int *evals_out, int *status_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(grad_guard(c, "gp_fit_map"));
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "gp_fit_map: call b7_gp_set_data first");
  if (!theta0 || !lo || !hi || !theta_out) return b7_fail(c, B7_ERR_INVALID, "gp_fit_map: NULL argument");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_fit_map: %d response columns (the fit of one column is built)", c->ycols);
  const int d = c->dfit, n = d + 3;
  MapCall m{c, d, B7_OK, std::vector<double>(d), std::vector<double>(n), false};
  std::vector<double> g(n), trace;
  double f = NAN;
  int iters = 0, evals = 0, status = 0;
  const int rc = lbfgsb_run(map_fn, &m, n, theta0, lo, hi, opts, theta_out, &f, g.data(), &iters, &evals, &status,
                            c->map_trace_on ? &trace : nullptr);
  if (m.rc != B7_OK) return m.rc;
  if (rc != B7_OK) return b7_fail(c, rc, "gp_fit_map: theta0 must be finite and inside [lo, hi], with lo <= hi");
  // the context's slot holds the fit of the LAST evaluation: where that was not theta_out (a rejected trial point came last), fit
  // theta_out once more -- the same call on the same numbers, so the same bits as the evaluation that produced f and g
  if (!m.last_ok || memcmp(m.last.data(), theta_out, sizeof(double) * n) != 0) {
    b7_hyp h;
    map_hyp(&m, theta_out, &h);
    double jitter = 0.0;
    int info = 0;
    B7_TRY(b7_gp_fit_hyp_grad(c, &h, &f, g.data(), &jitter, &info));
    evals += 1;
  }
  if (nll_out) *nll_out = f;
  if (grad_out) memcpy(grad_out, g.data(), sizeof(double) * n);
  if (iters_out) *iters_out = iters;
  if (evals_out) *evals_out = evals;
  if (status_out) *status_out = status;
  if (c->map_trace_on) {
    c->map_trace.swap(trace);
    c->map_trace_w = n + 2, c->map_trace_n = (int)(c->map_trace.size() / (size_t)(n + 2));
  }
  return B7_OK;
}

int b7_gp_fit_map_trace_enable(b7_ctx *c, int on) {
  if (!c) return B7_ERR_INVALID;
  c->map_trace_on = on != 0;
  c->map_trace.clear();
  c->map_trace_n = 0, c->map_trace_w = 0;
  return B7_OK;
}

int b7_gp_fit_map_trace(b7_ctx *c, double *records, int *n_records, int *width) {
  if (!c) return B7_ERR_INVALID;
  if (!n_records) return b7_fail(c, B7_ERR_INVALID, "gp_fit_map_trace: n_records is NULL");
  if (!c->map_trace_on || c->map_trace_w == 0) return b7_fail(c, B7_ERR_STATE, "gp_fit_map_trace: no traced b7_gp_fit_map on this context");
  *n_records = c->map_trace_n;
  if (width) *width = c->map_trace_w;
  if (records) memcpy(records, c->map_trace.data(), sizeof(double) * c->map_trace.size());
  return B7_OK;
}

}  // extern "C"

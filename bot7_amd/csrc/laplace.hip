// A probit Gaussian-process classifier by Laplace's method: the producer of log Pr[feasible | x] for constraints that are observed
// only as "it failed here" (Gelbart, Snoek & Adams 2014, section 2.3; Rasmussen & Williams 2006, algorithms 3.1 / 3.2).
//
// Labels v_i in {0, 1}, v = 1 meaning VIOLATED; s_i = 2 v_i - 1; Pr[v = 1 | h] = Phi(h).  With the mode f^ of the latent's posterior,
// W = -dd log p(v | f^) (diagonal), B = I + W^1/2 K W^1/2 = L L', a = d log p(v | f^), the latent posterior at a candidate is
//   mu* = mean + k*' a,     var* = amp - |(L^-1 W^1/2) k*|^2
// which is the regressor's posterior with Linv := L^-1 W^1/2 and alpha := a: a fit written into a FitSet slot is read unchanged by
// every posterior kernel (kpost_small_kernel, the K* / variance kernels, b7_gp_predict_at).  The new device code is the fit.
//
// laplace_small_kernel<MODE>: one fit per workgroup, the WHOLE Newton iteration inside the launch -- convergence and step decisions
// included, no host round trip inside a fit; B fits are B workgroups of one launch with no communication between them.  K(X,X) (no
// diagonal term) and the scaled observations of the B hyper vectors come from the existing assembly (launch_kxx_batch / launch_kxx with
// zero noise) one launch boundary ahead, so both covariance kernels and every d the general fit takes are served by one instance; the
// kernel reads K's lower triangle (what the regressor factors) and mirrors it.  MODE 0: the evidence only; MODE 1: also Linv and alpha.
//
// The rule (tests/_laplace_ref.py states it in float64):
//   start       a = 0, f = mean 1, psi(a, f) = -a'(f - mean)/2 + sum log Phi(s_i f_i)
//   it = 1..32  rho = phi/Phi at s f, g = s rho, W = max(rho (rho + s f), 0); B = I + W^1/2 K W^1/2 = L L'; b = W (f - mean) + g;
//               a+ = b - W^1/2 L^-T L^-1 W^1/2 K b; delta = |a+ - a|_inf.  delta <= 2^-26 max(1, |a+|_inf): take a+ whole and stop
//               (Newton is quadratic: that last step lands at rounding level).  Otherwise t = 1, 1/2, .., 2^-10: the first t with
//               psi(a + t (a+ - a)) >= psi(a), the last one if none.  Always f = mean + K a.
//   afterwards  rho, W, B, L again at f^;  Linv = L^-1 W^1/2, alpha = a, nll = -(psi(a, f^) - sum log L_ii), the iteration count, and
//               the "not converged within 32" bit (results are delivered all the same).
// B has every eigenvalue >= 1: no pivot fails, there is no jitter schedule and no redo path.
//
// Arithmetic.  The factorisation of B lives in LDS ([Npad + 1][Npad + 1] doubles: an odd row stride, so that a column read by
// consecutive rows and a row read by consecutive columns are both conflict-free): left-looking by columns, thread i owning row i and
// forming B_ij - sum_k L_ik L_jk as one ascending fma chain; every thread forms the pivot's chain redundantly (broadcast reads, the
// same bits), so a column costs ONE barrier.  The right-hand side rides along as row N of the same matrix (its "factor" row is
// L^-1 r: the forward substitution for free); the backward substitution runs in one wave without barriers.  Every sum has one fixed
// order (ascending fma chains per thread; reductions by a butterfly within wave 0): the same call twice gives the same bits, and a
// fit's bits depend neither on B, nor on its position in the batch, nor on the grid.  The explicit inverse (MODE 1) is formed in place,
// row by row.  This is the simple schedule: the 64 x 64 diagonal blocks through b7diag::diag_core and gs_body's 2 x 2 block scheme
// (MFMA) are the next step, not built here.
//
// Limits: N <= 128 (Npad 64 or 128), one response column.  256 threads; no scratch.  LDS: ((Npad + 1)^2 + 12 * 128 + 136) doubles =
// 143.1 KiB at Npad = 128, 46.1 KiB at Npad = 64 (one workgroup per CU either way at 128, three at 64).
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include "b7_internal.h"
#include "probit_math.h"

namespace {

constexpr int LAP_ITMAX = 32;       // Newton iterations
constexpr int LAP_HALVINGS = 10;    // t = 1, 1/2, .., 2^-10
constexpr int LAP_VEC = 12;         // [128] vectors in LDS
constexpr int LAP_THREADS = 256;

__host__ __device__ constexpr int lap_lds_doubles(int npad) { return (npad + 1) * (npad + 1) + LAP_VEC * 128 + 136; }

struct LapArgs {
  double *K;               // [B][npad][npad]; the lower triangle is read, the upper one rewritten as its mirror
  long long sK;
  const double *y;         // N labels, 0 or 1 (checked by the host)
  const double *mean_dev;  // B means, or null: mean0
  double mean0;
  int N, npad;
  double *out;             // [B][4]: nll, iterations, info, psi
  double *Linv, *alpha;    // MODE 1: [B][npad][npad], [B][npad]
  double *mode;            // nullable: [B][3][npad] f | a | W
};

// sum of v over the threads tid < 128 (the others' v is ignored), the same value on every thread: two halves added, then wave 0's
// butterfly.  tmp: 136 doubles.  Three barriers.
__device__ __forceinline__ double wg_sum(double v, double *tmp) {
  const int tid = threadIdx.x;
  if (tid < 128) tmp[tid] = v;
  __syncthreads();
  if (tid < 64) {
    double s = tmp[tid] + tmp[tid + 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (tid == 0) tmp[128] = s;
  }
  __syncthreads();
  const double r = tmp[128];
  __syncthreads();
  return r;
}
// ... and the maximum (of non-negative values; a NaN anywhere gives NaN: the comparison below then fails and the step is not "converged")
__device__ __forceinline__ double wg_max(double v, double *tmp) {
  const int tid = threadIdx.x;
  if (tid < 128) tmp[tid] = v;
  __syncthreads();
  if (tid < 64) {
    const double p = tmp[tid], q = tmp[tid + 64];
    double s = (p != p || q != q) ? NAN : (p > q ? p : q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double u = __shfl_xor(s, o);
      s = (s != s || u != u) ? NAN : (s > u ? s : u);
    }
    if (tid == 0) tmp[128] = s;
  }
  __syncthreads();
  const double r = tmp[128];
  __syncthreads();
  return r;
}

// out[i] = base + sum_j K[j][i] v[j], i < N: one ascending fma chain per thread over the mirrored matrix (row j is read by consecutive
// threads: coalesced).  The caller's barrier orders v before and out after.
__device__ __forceinline__ void matvec(const double *__restrict__ K, int npad, int N, const double *v, double base, double *out) {
  const int i = threadIdx.x;
  if (i < N) {
    double acc = 0.0;
#pragma unroll 8
    for (int j = 0; j < N; ++j) acc = __builtin_fma(K[(size_t)j * npad + i], v[j], acc);
    out[i] = base + acc;
  }
}

// the likelihood pieces at f: W, W^1/2 and (b != null) b = W (f - mean) + g
__device__ __forceinline__ void pieces(int N, const double *s, const double *f, double mean, double *W, double *sw, double *b) {
  const int i = threadIdx.x;
  if (i < 128) {
    double w = 0.0, bb = 0.0;
    if (i < N) {
      const double z = s[i] * f[i];
      const double rho = b7_probit_ratio(z);
      w = b7_probit_w(z, rho);
      bb = (w * (f[i] - mean)) + (s[i] * rho);
    }
    W[i] = w;
    sw[i] = sqrt(w);
    if (b) b[i] = bb;
  }
}

// psi(a, f) = -a'(f - mean)/2 + sum log Phi(s f)
__device__ __forceinline__ double psi_of(int N, const double *s, const double *a, const double *f, double mean, double *tmp) {
  const int i = threadIdx.x;
  double t = 0.0;
  if (i < N) t = ((a[i] * (f[i] - mean)) * -0.5) + b7_probit_logcdf(s[i] * f[i]);
  return wg_sum(t, tmp);
}

// A (lower, rows 0 .. N - 1) = I + W^1/2 K W^1/2; a wave per row, its lanes along the row
__device__ __forceinline__ void build_B(const double *__restrict__ K, int npad, int N, int LD, const double *sw, double *A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < N; i += LAP_THREADS / 64) {
    const double si = sw[i];
    for (int j = lane; j <= i; j += 64) {
      const double v = (si * K[(size_t)i * npad + j]) * sw[j];
      A[i * LD + j] = (i == j) ? v + 1.0 : v;
    }
  }
}

// rows 0 .. R - 1 (R = N, or N + 1 with a right-hand side in row N) of A against its first N columns: L below the diagonal in place,
// the pivots in dg, the diagonal of A left as it was.  Ends with a barrier.
__device__ __forceinline__ void factor(double *A, int LD, int N, int R, double *dg) {
  const int i = threadIdx.x;
  for (int j = 0; j < N; ++j) {
    if (i >= j && i < R) {
      const double *ri = A + i * LD, *rj = A + j * LD;
      double sv = ri[j], sd = rj[j];
#pragma unroll 4
      for (int k = 0; k < j; ++k) {
        const double lj = rj[k];
        sv = __builtin_fma(-ri[k], lj, sv);
        sd = __builtin_fma(-lj, lj, sd);
      }
      const double d = sqrt(sd);
      if (i == j) dg[j] = d;
      else A[i * LD + j] = sv / d;
    }
    __syncthreads();
  }
}

template <int MODE>
__global__ void __launch_bounds__(LAP_THREADS) laplace_small_kernel(LapArgs p) {
  extern __shared__ __align__(16) double sm[];
  const int tid = threadIdx.x, lane = tid & 63, fit = blockIdx.x;
  const int N = p.N, npad = p.npad, LD = npad + 1;
  double *A = sm;                       // [npad + 1][LD]
  double *va = A + (npad + 1) * LD;     // a
  double *vf = va + 128;                // f
  double *vn = vf + 128;                // a+
  double *vb = vn + 128;                // b
  double *vc = vb + 128;                // K b
  double *vW = vc + 128;
  double *vsw = vW + 128;
  double *vs = vsw + 128;               // s = 2 v - 1 (0 in the padding)
  double *vx = vs + 128;                // the solve's result
  double *vt = vx + 128;                // trial a
  double *vft = vt + 128;               // trial f
  double *dg = vft + 128;               // pivots
  double *tmp = dg + 128;               // [136] reductions
  double *K = p.K + (size_t)fit * p.sK;
  const double mean = p.mean_dev ? p.mean_dev[fit] : p.mean0;

  // K's upper triangle := its lower one (the kernel that assembled it rounds (i, j) and (j, i) apart; the regressor reads the lower)
  for (int i = tid >> 6; i < N; i += LAP_THREADS / 64)
    for (int j = lane; j < i; j += 64) K[(size_t)j * npad + i] = K[(size_t)i * npad + j];
  if (tid < 128) {
    va[tid] = 0.0;
    vf[tid] = tid < N ? mean : 0.0;
    vs[tid] = tid < N ? (2.0 * p.y[tid]) - 1.0 : 0.0;
  }
  __syncthreads();  // (workgroup scope: the mirrored entries are visible to this workgroup's loads)
  double psi = psi_of(N, vs, va, vf, mean, tmp);
  int iters = 0, converged = 0;
  for (int it = 1; it <= LAP_ITMAX && !converged; ++it) {
    iters = it;
    pieces(N, vs, vf, mean, vW, vsw, vb);
    __syncthreads();
    matvec(K, npad, N, vb, 0.0, vc);
    build_B(K, npad, N, LD, vsw, A);
    __syncthreads();
    if (tid < N) A[N * LD + tid] = vsw[tid] * vc[tid];  // r = W^1/2 K b, as row N
    __syncthreads();
    factor(A, LD, N, N + 1, dg);  // row N is now y = L^-1 r
    if (tid < 64) {
      // L' x = y, x_j for j descending; lane l holds entries l and l + 64 of what is left of y
      double v0 = lane < N ? A[N * LD + lane] : 0.0, v1 = lane + 64 < N ? A[N * LD + lane + 64] : 0.0;
      for (int j = N - 1; j >= 0; --j) {
        const double xj = __shfl(j >= 64 ? v1 : v0, j & 63) / dg[j];
        if (lane < j) v0 = __builtin_fma(-A[j * LD + lane], xj, v0);
        if (lane + 64 < j) v1 = __builtin_fma(-A[j * LD + lane + 64], xj, v1);
        if (lane == (j & 63)) vx[j] = xj;
      }
    }
    __syncthreads();
    double da = 0.0, na = 0.0;
    if (tid < N) {
      const double an = vb[tid] - (vsw[tid] * vx[tid]);
      vn[tid] = an;
      da = fabs(an - va[tid]);
      na = fabs(an);
    }
    const double delta = wg_max(da, tmp), nrm = wg_max(na, tmp);
    if (delta <= 3.7252902984619140625e-09 * (nrm > 1.0 ? nrm : 1.0)) {  // 2^-26
      converged = 1;
      if (tid < N) va[tid] = vn[tid];
      __syncthreads();
      matvec(K, npad, N, va, mean, vf);
      __syncthreads();
      psi = psi_of(N, vs, va, vf, mean, tmp);
      break;
    }
    double t = 1.0;
    for (int h = 0; h <= LAP_HALVINGS; ++h, t *= 0.5) {
      if (tid < N) vt[tid] = va[tid] + (t * (vn[tid] - va[tid]));
      __syncthreads();
      matvec(K, npad, N, vt, mean, vft);
      __syncthreads();
      const double pt = psi_of(N, vs, vt, vft, mean, tmp);
      if (pt >= psi || h == LAP_HALVINGS) {
        psi = pt;
        break;
      }
    }
    if (tid < N) {
      va[tid] = vt[tid];
      vf[tid] = vft[tid];
    }
    __syncthreads();
  }
  // ---- at the mode: W, B, L once more
  pieces(N, vs, vf, mean, vW, vsw, nullptr);
  __syncthreads();
  build_B(K, npad, N, LD, vsw, A);
  __syncthreads();
  factor(A, LD, N, N, dg);
  const double ld = wg_sum(tid < N ? log(dg[tid]) : 0.0, tmp);
  if (tid == 0) {
    double *o = p.out + 4 * (size_t)fit;
    o[0] = -(psi - ld);
    o[1] = (double)iters;
    o[2] = converged ? 0.0 : 1.0;
    o[3] = psi;
  }
  if (p.mode && tid < npad) {
    double *m = p.mode + (size_t)fit * 3 * npad;
    m[tid] = tid < N ? vf[tid] : 0.0;
    m[npad + tid] = tid < N ? va[tid] : 0.0;
    m[2 * npad + tid] = tid < N ? vW[tid] : 0.0;
  }
  if constexpr (MODE == 1) {
    // X = L^-1 in place, rows ascending: X_ic = (e_ic - sum_{c <= k < i} L_ik X_kc) / L_ii; thread c owns column c.  A row's reads of L
    // and its writes of X are a barrier apart; a column's earlier X entries are the owning thread's own writes.
    for (int i = 0; i < N; ++i) {
      double val = 0.0;
      if (tid <= i) {
        double acc = 0.0;
        for (int k = tid; k < i; ++k) acc = __builtin_fma(A[i * LD + k], A[k * LD + tid], acc);
        val = (tid == i) ? 1.0 / dg[i] : (-acc) / dg[i];
      }
      __syncthreads();
      if (tid <= i) A[i * LD + tid] = val;
    }
    __syncthreads();
    double *Li = p.Linv + (size_t)fit * npad * npad;
    const int sh = npad == 128 ? 7 : 6;
    for (int e = tid; e < npad * npad; e += LAP_THREADS) {
      const int i = e >> sh, j = e & (npad - 1);
      Li[e] = (i < N && j <= i) ? A[i * LD + j] * vsw[j] : 0.0;
    }
    if (tid < npad) p.alpha[(size_t)fit * npad + tid] = tid < N ? va[tid] : 0.0;
  }
}

template <int MODE>
int lap_launch(b7_ctx *c, int B, const LapArgs &a) {
  const size_t lds = sizeof(double) * (size_t)lap_lds_doubles(a.npad);
  static bool attr_done[64] = {false};  // the opt-in to > 64 KiB of dynamic LDS: once per instantiation AND device
  if (c->device >= 64 || !attr_done[c->device]) {
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(laplace_small_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(double) * (size_t)lap_lds_doubles(128))));
    if (c->device < 64) attr_done[c->device] = true;
  }
  hipLaunchKernelGGL(laplace_small_kernel<MODE>, dim3(B), dim3(LAP_THREADS), lds, c->stream, a);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

__global__ void __launch_bounds__(256) add_const_kernel(const double *__restrict__ src, double *__restrict__ dst, long long n, double v) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) dst[e] = src[e] + v;
}

__global__ void __launch_bounds__(256) probit_kernel(const double *__restrict__ z, long long n, double *logcdf, double *ratio, double *w) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) {
    const double rho = b7_probit_ratio(z[e]);
    logcdf[e] = b7_probit_logcdf(z[e]);
    ratio[e] = rho;
    w[e] = b7_probit_w(z[e], rho);
  }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------
// what every classifier entry point refuses, by code and name; labels: checked once per data set (the epoch moves with the data)
static inline bool fin(double x) { return x - x == 0.0; }

int clf_guard(b7_ctx *c, const char *who) {
  if (c->group) return b7_fail(c, B7_ERR_STATE, "%s: this context belongs to a group (the classifier over a sharded grid is not built)", who);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: a communicator of %d ranks (the classifier over a sharded grid is not built)", who, c->comm_world);
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "%s: call b7_gp_set_data first", who);
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: %d response columns (one column of 0 / 1 labels is built)", who, c->ycols);
  if (c->N > 128)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: N = %d > 128 observations (the Laplace fit on the general schedule is not built)", who, c->N);
  B7_HIP(c, hipSetDevice(c->device));
  if (c->clf_lab_epoch != c->epoch || c->clf_lab_N != c->N) {
    double lab[128];
    B7_HIP(c, hipMemcpyAsync(lab, c->ybuf.p, sizeof(double) * c->N, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    c->clf_lab_bad = 0;
    for (int i = 0; i < c->N && !c->clf_lab_bad; ++i)
      if (!(lab[i] == 0.0 || lab[i] == 1.0)) c->clf_lab_bad = i + 1;
    c->clf_lab_epoch = c->epoch, c->clf_lab_N = c->N;
  }
  if (c->clf_lab_bad)
    return b7_fail(c, B7_ERR_INVALID, "%s: label %d is not exactly 0 or 1 (1 = the constraint is violated)", who, c->clf_lab_bad - 1);
  return B7_OK;
}

int clf_check_hyp(b7_ctx *c, const char *who, const b7_hyp *h, int s) {
  if (!h->lenscale_sq) return b7_fail(c, B7_ERR_INVALID, "%s: NULL lenscale_sq (fit %d)", who, s);
  for (int k = 0; k < c->dfit; ++k)
    if (!(h->lenscale_sq[k] > 0.0) || !fin(h->lenscale_sq[k]))
      return b7_fail(c, B7_ERR_INVALID, "%s: lenscale_sq[%d] must be > 0 and finite (fit %d)", who, k, s);
  if (!(h->amp > 0.0) || !fin(h->amp) || !fin(h->noise) || !fin(h->mean))
    return b7_fail(c, B7_ERR_INVALID, "%s: amp > 0, and amp, noise (ignored) and mean finite (fit %d)", who, s);
  return B7_OK;
}

// S fits side by side: the hypers packed (noise := 0: the probit link has unit variance and K takes no diagonal term) through pinned
// memory into c->bhyp, the operands and K of every fit by the regressor's assembly, then one launch of S workgroups.  with_fit: Linv
// and alpha into the batch slots (batch_fits(c, S) afterwards).  The [S][4] results are on their way to `res` (pinned) on return.
int clf_fits(b7_ctx *c, const char *who, int S, const b7_hyp *hyps, bool with_fit, double **res) {
  const int d = c->dfit, n = c->Npad;
  for (int s = 0; s < S; ++s) B7_TRY(clf_check_hyp(c, who, &hyps[s], s));
  const size_t hyp_doubles = (size_t)S * (d + 3);
  B7_TRY(b7_pin_ensure(c, c->pin_nll, sizeof(double) * (hyp_doubles + 4 * (size_t)S) + 64, true));
  B7_TRY(b7_ensure(c, c->bhyp, sizeof(double) * hyp_doubles));
  B7_TRY(batch_slots_ensure(c, S, B7_SLOTS_OPERANDS | (with_fit ? B7_SLOTS_LINV | B7_SLOTS_ALPHA : 0)));
  B7_TRY(b7_ensure(c, c->bK, sizeof(double) * (size_t)S * n * n));
  B7_TRY(b7_ensure(c, c->clf, sizeof(double) * 4 * (size_t)S));
  double *pack = static_cast<double *>(c->pin_nll.host);
  const HypPack hp = hyp_pack(pack, S, d);
  for (int s = 0; s < S; ++s) {
    memcpy(hp.ls + (size_t)s * d, hyps[s].lenscale_sq, sizeof(double) * d);
    hp.amp[s] = hyps[s].amp, hp.noise[s] = 0.0, hp.mean[s] = hyps[s].mean;
  }
  B7_HIP(c, hipMemcpyAsync(c->bhyp.p, pack, sizeof(double) * hyp_doubles, hipMemcpyHostToDevice, c->stream));
  const HypPack hd = hyp_pack(c->bhyp.p, S, d);
  B7_TRY(launch_kxx_batch(c, S, hd.ls, hd.amp, hd.noise, (double *)c->bw.p, (double *)c->bzsc.p, (double *)c->bzss.p, (double *)c->bK.p));
  B7_TRY(launch_laplace_small(c, S, (double *)c->bK.p, (int64_t)n * n, hd.mean, 0.0, (double *)c->clf.p, with_fit ? (double *)c->bLinv.p : nullptr,
                              with_fit ? (double *)c->balpha.p : nullptr, nullptr));
  *res = pack + hyp_doubles;
  B7_HIP(c, hipMemcpyAsync(*res, c->clf.p, sizeof(double) * 4 * (size_t)S, hipMemcpyDeviceToHost, c->stream));
  return B7_OK;
}

void clf_report(const double *res, int S, double *nll_out, int *iters_out, int *info_out) {
  for (int s = 0; s < S; ++s) {
    if (nll_out) nll_out[s] = res[4 * s];
    if (iters_out) iters_out[s] = (int)res[4 * s + 1];
    if (info_out) info_out[s] = (int)res[4 * s + 2];
  }
}

}  // namespace

int launch_laplace_small(b7_ctx *c, int B, double *K, int64_t sK, const double *mean_dev, double mean0, double *out, double *Linv,
                         double *alpha, double *mode) {
  PhaseScope ps(c, "laplace");
  if (B < 1 || c->N < 1 || c->N > 128 || (c->Npad != 64 && c->Npad != 128) || c->N > c->Npad || (Linv == nullptr) != (alpha == nullptr))
    return b7_fail(c, B7_ERR_INVALID, "laplace: B %d N %d Npad %d outside the one-workgroup fit", B, c->N, c->Npad);
  LapArgs a = {};
  a.K = K, a.sK = sK, a.y = (const double *)c->ybuf.p, a.mean_dev = mean_dev, a.mean0 = mean0;
  a.N = c->N, a.npad = c->Npad, a.out = out, a.Linv = Linv, a.alpha = alpha, a.mode = mode;
  return Linv ? lap_launch<1>(c, B, a) : lap_launch<0>(c, B, a);
}

extern "C" {

int b7_clf_nll_batch(b7_ctx *c, int B, const b7_hyp *hyps, double *nll_out, int *iters_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(clf_guard(c, "clf_nll_batch"));
  if (B < 1 || !hyps || !nll_out) return b7_fail(c, B7_ERR_INVALID, "clf_nll_batch: B >= 1, hyps and nll_out required");
  double *res = nullptr;
  B7_TRY(clf_fits(c, "clf_nll_batch", B, hyps, false, &res));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  clf_report(res, B, nll_out, iters_out, info_out);
  return B7_OK;
}

int b7_clf_fit_hyp(b7_ctx *c, const b7_hyp *hyp, double *nll_out, int *iters_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(clf_guard(c, "clf_fit_hyp"));
  if (!hyp) return b7_fail(c, B7_ERR_INVALID, "clf_fit_hyp: hyp is NULL");
  B7_TRY(clf_check_hyp(c, "clf_fit_hyp", hyp, 0));
  const int d = c->dfit, n = c->Npad;
  c->clf_mode_valid = false;
  B7_TRY(b7_ensure(c, c->clf, sizeof(double) * 4));
  B7_TRY(b7_ensure(c, c->clf_mode, sizeof(double) * 3 * (size_t)n));
  // the fit's front end is the regressor's, with no noise on K's diagonal: lengthscales through the pinned block's vector slot into the
  // scratch block (where b7_gp_fit_hyp leaves them), observation scaling, K(X,X) into the context's own slot
  double *ls_stage = c->pinned->vec, *ls_dev = b7_scratch(c)->lenscale;
  memcpy(ls_stage, hyp->lenscale_sq, sizeof(double) * d);
  B7_HIP(c, hipMemcpyAsync(ls_dev, ls_stage, sizeof(double) * d, hipMemcpyHostToDevice, c->stream));
  const b7_hyp h0{hyp->lenscale_sq, hyp->amp, 0.0, hyp->mean};
  B7_TRY(fit_front(c, &h0, ls_dev));
  B7_TRY(launch_laplace_small(c, 1, (double *)c->K.p, 0, nullptr, hyp->mean, (double *)c->clf.p, (double *)c->Linv.p, (double *)c->alpha.p,
                              (double *)c->clf_mode.p));
  double *res = c->pinned->fit.terms;
  B7_HIP(c, hipMemcpyAsync(res, c->clf.p, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  clf_report(res, 1, nll_out, iters_out, info_out);
  c->linv_done = true;
  c->fitted = true;  // the latent's fit: b7_gp_predict / b7_gp_predict_at return its mean and variance
  c->clf_mode_valid = true, c->clf_epoch = c->epoch, c->clf_N = c->N;
  return B7_OK;
}

int b7_clf_mode_get(b7_ctx *c, double *f_out, double *a_out, double *W_out) {
  if (!c) return B7_ERR_INVALID;
  if (!c->clf_mode_valid || c->clf_epoch != c->epoch)
    return b7_fail(c, B7_ERR_STATE, "clf_mode_get: no Laplace fit on this context (call b7_clf_fit_hyp; a change of the data or the covariance kernel forgets it)");
  B7_HIP(c, hipSetDevice(c->device));
  const size_t nb = sizeof(double) * (size_t)c->clf_N, n = (size_t)c->Npad;
  const double *m = (const double *)c->clf_mode.p;
  if (f_out) B7_HIP(c, hipMemcpyAsync(f_out, m, nb, hipMemcpyDeviceToHost, c->stream));
  if (a_out) B7_HIP(c, hipMemcpyAsync(a_out, m + n, nb, hipMemcpyDeviceToHost, c->stream));
  if (W_out) B7_HIP(c, hipMemcpyAsync(W_out, m + 2 * n, nb, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_clf_eval_logfeas(b7_ctx *c, int S, const b7_hyp *hyps, double *best_val, int64_t *best_idx1, int *iters_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(clf_guard(c, "clf_eval_logfeas"));
  if (S < 1 || !hyps || !best_val || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "clf_eval_logfeas: S >= 1, hyps, best_val and best_idx1 required");
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "clf_eval_logfeas: no candidate grid on this context");
  if (c->d != c->dfit) return b7_fail(c, B7_ERR_INVALID, "clf_eval_logfeas: grid dims %d != data dims %d", c->d, c->dfit);
  for (int s = 0; s < S; ++s) B7_TRY(clf_check_hyp(c, "clf_eval_logfeas", &hyps[s], s));  // (before anything is given up)
  const int64_t M = c->M;
  const size_t SM = (size_t)S * (size_t)M;
  c->post_valid = false;
  B7_TRY(b7_ensure(c, c->post, sizeof(double) * 2 * SM));
  B7_TRY(b7_ensure(c, c->bvar, sizeof(double) * SM));
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)M));
  double *res = nullptr;
  B7_TRY(clf_fits(c, "clf_eval_logfeas", S, hyps, true, &res));
  // the latent posterior of every sample over the resident grid, kept as b7_eval_posterior keeps one (b7_posterior_get serves it): the
  // route the regressor's nomination takes for this shape
  double *pmu = (double *)c->post.p, *pvar = pmu + SM;
  const double *grid = (const double *)c->grid[c->grid_cur].p;
  const FitSet fits = batch_fits(c, S);
  c->model_kind = 0;
  c->fitted = false;  // the context's own fit slot holds none of these samples, as after b7_eval_nominate
  c->predicted = false;
  c->clf_mode_valid = false;
  if (c->kpost_small && kpost_small_applies(c)) {
    B7_TRY(launch_kpost_small(c, fits, grid, M, pmu, pvar, M));
  } else {
    for (int s = 0; s < S; ++s)
      B7_TRY(predict_into(c, fit_at(fits, s, b7_hyp{nullptr, hyps[s].amp, 0.0, hyps[s].mean}), grid, M, pmu + (size_t)s * M, pvar + (size_t)s * M));
  }
  // log Phi((0 - mu) / sqrt(var + 1)) per sample -- the LogPI piece at threshold 0 with the probit link's unit variance added, this
  // entry point's own + 1 -- marginalised by log-sum-exp in sample order, score:div and the arg-max: b7_eval_nominate's last launch
  hipLaunchKernelGGL(add_const_kernel, dim3((unsigned)((SM + 255) / 256)), dim3(256), 0, c->stream, (const double *)pvar, (double *)c->bvar.p,
                     (long long)SM, 1.0);
  B7_HIP(c, hipGetLastError());
  ScoreParams pend;
  pend.kind = B7_SCORE_LOGPI, pend.S = S, pend.mu = pmu, pend.var = (const double *)c->bvar.p, pend.stride = M;
  pend.fmin = nullptr, pend.fmin0 = 0.0, pend.tradeoff = 0.0;
  acc_declare_zeros(c, B7_SCORE_LOGPI);
  B7_TRY(exch_local(c, (double)S, 0, 0, 1, true, true, &pend));
  B7_TRY(exch_wait_mirror(c));  // one stream: the fits' reports, enqueued earlier, have landed too
  clf_report(res, S, nullptr, iters_out, info_out);
  c->post_S = S, c->post_M = M, c->post_valid = true;
  return exch_conclude(c, c->tab_host, 1, best_val, best_idx1);
}

int b7_probit_compute(b7_ctx *c, const double *z, int64_t n, double *logcdf_out, double *ratio_out, double *w_out) {
  if (!c) return B7_ERR_INVALID;
  if (n < 0 || (n > 0 && (!z || !logcdf_out || !ratio_out || !w_out))) return b7_fail(c, B7_ERR_INVALID, "probit_compute: bad arguments");
  if (n == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->clf_user, sizeof(double) * 4 * (size_t)n));
  double *zd = (double *)c->clf_user.p, *o = zd + n;
  B7_HIP(c, hipMemcpyAsync(zd, z, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(probit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double *)zd, (long long)n, o, o + n, o + 2 * n);
  B7_HIP(c, hipGetLastError());
  B7_HIP(c, hipMemcpyAsync(logcdf_out, o, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(ratio_out, o + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(w_out, o + 2 * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

}  // extern "C"

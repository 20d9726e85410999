// Thompson nominees refined off the grid by descent on their own sample paths -- b7_ts_nominate_refine, b7_ts_path_grad_at.
//
// No counterpart in the reference.  A pathwise sample (Wilson et al. 2020, rff.hip) is an explicit differentiable function of x:
//   f_j(x)     = m_s + sum_f W_j[f] cos(omega_s[f] . x + phase[f]) + sum_i v_j[i] k_s(x, X_i)            s = j mod S
//   df_j/dx_c  = -sum_f W_j[f] sin(omega_s[f] . x + phase[f]) omega_s[f][c] - w_c (x_c sum_i v_j[i] g_i - sum_i v_j[i] g_i X_ic)
// W = sqrt(2 amp / F) weight, w_c = 1 / lenscale_sq_c, g the radial factor of cov_grad_nonpos4<KERN>.  No L^-1, no variance and no
// hyper-sample loop: one evaluation is O((F + N) d) per point.  Every operand is what the last b7_ts_nominate left (ts_kept).
//
// ts_refine_kernel<KERN, DPAD>: value and gradient at 16 query columns per wave (column = 4 start + rung) on the fp64 matrix cores,
// rff_kernel's fragment chain (gemm_f64.h's maps):
//   per 16 features   D = Omega chunk x X' (DPAD / 4 MFMAs), + phase and sine / cosine in place; the value is a per-lane sum of
//                     W cos; G[c][col] -= sum_f omega[f][c] (W_f sin_f[col]): Omega' as the A operand, the scaled D registers as B;
//   per 16 obs.       the same chain: the distance argument of refine_k_kernel ((c - xs/2) - zs/2), k and g from
//                     cov_grad_nonpos4<KERN>, the value sum v_i k_i; the scaled observations transposed as A, (v_i g_i)[col] as B;
//                     the x_c w_c sum v_i g_i term from the per-lane sums.
// A gradient entry G[c][col] lands in lane 16 (c mod 4) + col, register c / 4: the lane and slot that holds x_c of the same column
// as a B fragment, so the ladder's point update is lane-local; max_c |g~_c| is a reduction over the four 16-lane groups, and the
// taken rung reaches its start's four columns by a shuffle inside its quad.  The whole refinement of a start runs inside one
// launch: one wave owns four starts for all iterations; no launch, flag or barrier between iterations, no dependency across waves.
// One workgroup of four waves = the 16 starts of one path.  Every sum has one order, so a start's trajectory is a function of its
// path's operands, its start row and the options alone.
//
// The ladder is b7_eval_nominate_refine's (score.hip: refine_step_kernel) applied to -f_j: same rungs, same point formula in the
// same rounded operations, same decision rule, eta update, floor and status bits.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"
#include "gemm_f64.h"
#include "ksx_exp.h"

namespace {

constexpr int TS_PMAX = B7_REFINE_MAX_STARTS;  // starts of a path = the 16 columns x 4 waves / 4 rungs of its workgroup

// (sin x, cos x) for |x| < 2^30: rff_cos's reduction and polynomials (rff.hip), both quadrant selections
__device__ __forceinline__ void rff_sincos(double x, double *s_out, double *c_out) {
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
  // n mod 4 = 0: (sin r, cos r), 1: (cos r, -sin r), 2: (-sin r, -cos r), 3: (-cos r, sin r)
  const int k = (int)n;
  const double cv = (k & 1) ? sn : cs, sv = (k & 1) ? cs : sn;
  *c_out = ((k + 1) & 2) ? -cv : cv;
  *s_out = (k & 2) ? -sv : sv;
}

// The operands of a call in fragment order, zero padded (ts_pack_sample_kernel, ts_pack_path_kernel).  Per hyper sample s, at
// stride s_*: KS = DPAD / 4, NT = ceil(DPAD / 16), lr = lane & 15, lq = lane >> 4
//   omf[(ch KS + k4) 64 + lane]        = Omega[16 ch + lr][4 k4 + lq]                    the value's A operand (rff_pack_kernel's)
//   omt[((ch NT + ct) 4 + r) 64 + lane] = Omega[16 ch + 4 r + lq][16 ct + lr]             the gradient's: Omega transposed
//   zf[(t KS + k4) 64 + lane]          = X[16 t + lr][4 k4 + lq] w[4 k4 + lq]            observations scaled by w = 1 / lenscale_sq
//   zt[((t NT + ct) 4 + r) 64 + lane]  = X[16 t + 4 r + lq][16 ct + lr] w[16 ct + lr]
//   zss[i] = (sum_k X[i][k]^2 w[k]) / 2,  w[DPAD]
// per path j: Wp[j][f] = sqrt(2 amp / F) weight[j][f], vp[j][i] = v_j[i] (0 beyond N), par[j] = amp | mean
struct TsOps {
  const double *omf, *omt, *zf, *zt, *zss, *w;
  long long s_omf, s_omt, s_zf, s_zt, s_zss;
  const double *phase, *Wp, *vp, *par;
  int d, F, N, np16, S;
};

__global__ void __launch_bounds__(256) ts_pack_sample_kernel(const double *__restrict__ omega_, const double *__restrict__ xobs,
                                                             const double *__restrict__ hyp, int F, int d, int dpad, int N, int np16,
                                                             double *omf_, double *omt_, double *zf_, double *zt_, double *zss_,
                                                             double *w_) {
  const int s = blockIdx.y, KS = dpad / 4, NT = (dpad + 15) / 16;
  const double *omega = omega_ + (int64_t)s * F * d, *ls = hyp + (int64_t)s * (d + 3);
  double *omf = omf_ + (int64_t)s * F * dpad, *omt = omt_ + (int64_t)s * F * 16 * NT;
  double *zf = zf_ + (int64_t)s * np16 * dpad, *zt = zt_ + (int64_t)s * np16 * 16 * NT, *zss = zss_ + (int64_t)s * np16, *w = w_ + s * dpad;
  const int64_t n0 = (int64_t)F * dpad, n1 = n0 + (int64_t)F * 16 * NT, n2 = n1 + (int64_t)np16 * dpad, n3 = n2 + (int64_t)np16 * 16 * NT;
  const int64_t n4 = n3 + np16, n5 = n4 + dpad;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n5; e += (int64_t)gridDim.x * blockDim.x) {
    if (e < n0) {
      const int lane = (int)(e & 63);
      const int64_t t = e >> 6;
      const int k4 = (int)(t % KS), f = (int)(t / KS) * 16 + (lane & 15), k = 4 * k4 + (lane >> 4);
      omf[e] = k < d ? omega[(int64_t)f * d + k] : 0.0;
    } else if (e < n1) {
      const int64_t u = e - n0, t = u >> 6;
      const int lane = (int)(u & 63), r = (int)(t & 3), ct = (int)((t >> 2) % NT), ch = (int)((t >> 2) / NT);
      const int f = 16 * ch + 4 * r + (lane >> 4), cc = 16 * ct + (lane & 15);
      omt[u] = cc < d ? omega[(int64_t)f * d + cc] : 0.0;
    } else if (e < n2) {
      const int64_t u = e - n1, t = u >> 6;
      const int lane = (int)(u & 63), k4 = (int)(t % KS), i = (int)(t / KS) * 16 + (lane & 15), k = 4 * k4 + (lane >> 4);
      zf[u] = (i < N && k < d) ? xobs[(int64_t)i * d + k] * (1.0 / ls[k]) : 0.0;
    } else if (e < n3) {
      const int64_t u = e - n2, t = u >> 6;
      const int lane = (int)(u & 63), r = (int)(t & 3), ct = (int)((t >> 2) % NT), tt = (int)((t >> 2) / NT);
      const int i = 16 * tt + 4 * r + (lane >> 4), cc = 16 * ct + (lane & 15);
      zt[u] = (i < N && cc < d) ? xobs[(int64_t)i * d + cc] * (1.0 / ls[cc]) : 0.0;
    } else if (e < n4) {
      const int i = (int)(e - n3);
      double a = 0.0;
      if (i < N)
        for (int k = 0; k < d; ++k) {
          const double x = xobs[(int64_t)i * d + k];
          a = a + (x * x) * (1.0 / ls[k]);
        }
      zss[i] = 0.5 * a;
    } else {
      const int k = (int)(e - n4);
      w[k] = k < d ? 1.0 / ls[k] : 0.0;
    }
  }
}

__global__ void __launch_bounds__(256) ts_pack_path_kernel(const double *__restrict__ weight, const double *__restrict__ alpha,
                                                           long long alpha_stride, const double *__restrict__ hyp, int F, int d, int N,
                                                           int np16, int S, int q, double *Wp, double *vp, double *par) {
  const int j = blockIdx.y, s = j % S, p = j / S;
  const int qs = (q - s + S - 1) / S, yld = qs == 1 ? 1 : (qs + 63) / 64 * 64;
  const double *hs = hyp + (int64_t)s * (d + 3);
  const double scale = sqrt(2.0 * hs[d] / F);
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < F + np16 + 2; e += gridDim.x * blockDim.x) {
    if (e < F)
      Wp[(int64_t)j * F + e] = scale * weight[(int64_t)j * F + e];
    else if (e < F + np16) {
      const int i = e - F;
      vp[(int64_t)j * np16 + i] = i < N ? alpha[s * alpha_stride + (int64_t)i * yld + p] : 0.0;
    } else
      par[2 * j + (e - F - np16)] = (e - F - np16) ? hs[d + 2] : hs[d];
  }
}

__device__ __forceinline__ double quad16_sum(double v) {  // over the four 16-lane groups, the same bits in each
  v = v + __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// Value and gradient of path j at this wave's 16 columns: xb[k4] = x[4 k4 + lq] of column lr (a B fragment; 0 beyond d).
// -> val (the same in the four lanes of a column) and G[ct][r] = df/dx_c, c = 16 ct + 4 r + lq = 4 (4 ct + r) + lq: xb's slots
template <int KERN, int DPAD>
__device__ __forceinline__ void ts_eval16(const TsOps &o, int j, const double *__restrict__ stab, const double *__restrict__ sw,
                                          const double (&xb)[DPAD / 4], double *val_out, d4_t (&G)[(DPAD + 15) / 16]) {
  constexpr int KS = DPAD / 4, NT = (DPAD + 15) / 16;
  const int lane = threadIdx.x & 63, lq = lane >> 4, s = j % o.S;
  const double *omf = o.omf + s * o.s_omf, *omt = o.omt + s * o.s_omt, *zf = o.zf + s * o.s_zf, *zt = o.zt + s * o.s_zt;
  const double *zss = o.zss + s * o.s_zss, *Wp = o.Wp + (int64_t)j * o.F, *vp = o.vp + (int64_t)j * o.np16;
  double hq = 0.0;
#pragma unroll
  for (int k4 = 0; k4 < KS; ++k4) hq = hq + (xb[k4] * xb[k4]) * sw[4 * k4 + lq];
  hq = 0.5 * quad16_sum(hq);
  double vsum = 0.0, gsum = 0.0;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) G[ct] = d4_t{0.0, 0.0, 0.0, 0.0};
  const int nch = o.F / 16, nt = o.np16 / 16;
  for (int ch = 0; ch < nch; ++ch) {
    d4_t D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) D = mfma_f64(omf[((int64_t)ch * KS + k4) * 64 + lane], xb[k4], D);
    double b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = ch * 16 + 4 * r + lq;
      double sn, cs;
      rff_sincos(D[r] + o.phase[f], &sn, &cs);
      const double wv = Wp[f];
      vsum = __builtin_fma(wv, cs, vsum);
      b[r] = -(wv * sn);
    }
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) G[ct] = mfma_f64(omt[(((int64_t)ch * NT + ct) * 4 + r) * 64 + lane], b[r], G[ct]);
  }
  for (int t = 0; t < nt; ++t) {
    d4_t D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) D = mfma_f64(zf[((int64_t)t * KS + k4) * 64 + lane], xb[k4], D);
    double arg[4], kv[4], gv[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) arg[r] = (D[r] - hq) - zss[t * 16 + 4 * r + lq];
    cov_grad_nonpos4<KERN>(arg, stab, kv, gv);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = t * 16 + 4 * r + lq;
      const bool live = i < o.N;  // a padding observation gives exactly 0
      const double v = vp[i];
      vsum = __builtin_fma(v, live ? kv[r] : 0.0, vsum);
      b[r] = v * (live ? gv[r] : 0.0);
      gsum = gsum + b[r];
    }
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) G[ct] = mfma_f64(zt[(((int64_t)t * NT + ct) * 4 + r) * 64 + lane], b[r], G[ct]);
  }
  *val_out = o.par[2 * j + 1] + quad16_sum(vsum);
  gsum = quad16_sum(gsum);
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * ct + r < KS) G[ct][r] = G[ct][r] - (xb[4 * ct + r] * sw[4 * (4 * ct + r) + lq]) * gsum;
}

// the workgroup's tables: amp 2^(i/128) for the covariance, and w | lo | hi of the path's hyper sample and the box
template <int DPAD>
__device__ __forceinline__ void ts_tables(const TsOps &o, int j, const double *__restrict__ box, double *stab, double *sw, double *slo,
                                          double *shi) {
  const int tid = threadIdx.x;
  if (tid < 128) stab[tid] = o.par[2 * j] * b7_exp2_tab_dev[tid];
  if (tid < DPAD) {
    sw[tid] = o.w[(j % o.S) * DPAD + tid];
    slo[tid] = (box && tid < o.d) ? box[tid] : 0.0;
    shi[tid] = (box && tid < o.d) ? box[o.d + tid] : 0.0;
  }
  __syncthreads();
}

// What the refinement leaves: x, g [q][16][B7_MAX_D], v, eta [q][16], status [q][16]
struct TsRefOut {
  double *x, *g, *v;
  int *status;
  double *trace;  // nullable: [q][16][iters + 1][B7_REFINE_TRACE_WIDTH]
};

// block = path blockIdx.x, wave = its starts 4 wave .. 4 wave + 3, column lr = 4 (start in wave) + rung
template <int KERN, int DPAD>
__global__ void __launch_bounds__(256) ts_refine_kernel(TsOps o, const double *__restrict__ grid, const long long *__restrict__ starts,
                                                        const double *__restrict__ box, int P, int iters, double eta0, TsRefOut out) {
  constexpr int KS = DPAD / 4, NT = (DPAD + 15) / 16;
  __shared__ double stab[128], sw[DPAD], slo[DPAD], shi[DPAD];
  const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4, d = o.d;
  ts_tables<DPAD>(o, j, box, stab, sw, slo, shi);
  if (4 * wave >= P) return;  // wave-uniform; no barrier follows
  const int st = 4 * wave + (lr >> 2), rung = lr & 3, quad = lane & ~3;
  const long long row = st < P ? starts[j * TS_PMAX + st] : -1;
  const bool valid = row >= 0;
  double sx[KS], sg[KS], xb[KS];  // the start's point and gradient, the column's query: c = 4 k4 + lq
#pragma unroll
  for (int k4 = 0; k4 < KS; ++k4) {
    const int c = 4 * k4 + lq;
    sx[k4] = (valid && c < d) ? grid[row * d + c] : 0.0;
    sg[k4] = 0.0;
    xb[k4] = sx[k4];
  }
  double v = NAN, eta = eta0;
  int status = valid ? 0 : B7_REFINE_NOT_RUN;
  bool active = false;
  const double rk = rung == 0 ? 1.0 : rung == 1 ? 0.25 : rung == 2 ? 0.0625 : 0.015625;
  for (int it = 0; it <= iters; ++it) {
    double val;
    d4_t G[NT];
    ts_eval16<KERN, DPAD>(o, j, stab, sw, xb, &val, G);
    double cand[4] = {NAN, NAN, NAN, NAN}, eta_new = eta;
    int taken = -1;
    if (it == 0) {
      taken = 0;  // the start itself
      v = __shfl(val, quad);
      if (!(status & B7_REFINE_NOT_RUN) && !(fabs(v) < INFINITY)) status |= B7_REFINE_NOT_RUN;
    } else {
      double cq[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) cq[k] = __shfl(val, quad + k);
      if (active) {
        int kb = -1;
        double bv = 0.0;  // of -f: the highest, the lowest rung on ties, never a NaN
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cand[k] = cq[k];
          const double a = -cq[k];
          if (a == a && (kb < 0 || a > bv)) kb = k, bv = a;
        }
        if (kb >= 0 && bv > -v) {
          const double tk = eta * (kb == 0 ? 1.0 : kb == 1 ? 0.25 : kb == 2 ? 0.0625 : 0.015625);
          taken = kb, v = -bv, status |= B7_REFINE_MOVED;
          eta_new = (4.0 * tk < 1.0) ? 4.0 * tk : 1.0;
        } else {
          eta_new = eta / 256.0;
        }
        if (eta_new < 0x1p-40) status |= B7_REFINE_CONVERGED;
      }
    }
    // the taken rung's column to the start's four (every lane takes part in the shuffles)
    {
      const int src = quad + (taken >= 0 ? taken : 0);
#pragma unroll
      for (int k4 = 0; k4 < KS; ++k4) {
        const double nx = __shfl(xb[k4], src), ng = __shfl(G[k4 >> 2][k4 & 3], src);
        if (taken >= 0) sx[k4] = nx, sg[k4] = ng;
      }
    }
    // the next ladder on -f: g~ = -grad o (hi - lo), m = max |g~|
    bool next = it < iters && !(status & (B7_REFINE_NOT_RUN | B7_REFINE_CONVERGED));
    double m = 0.0;
    int bad = 0;
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) {
      const int c = 4 * k4 + lq;
      if (c < d) {
        const double a = fabs(-sg[k4] * (shi[c] + (-slo[c])));
        bad |= (a != a);
        if (a > m) m = a;
      }
    }
    m = fmax(m, __shfl_xor(m, 16)), bad |= __shfl_xor(bad, 16);
    m = fmax(m, __shfl_xor(m, 32)), bad |= __shfl_xor(bad, 32);
    if (next && (bad || m == 0.0 || !(m < INFINITY))) status |= B7_REFINE_FLAT, next = false;
    const double tk = eta_new * rk;
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) {
      const int c = 4 * k4 + lq;
      double x = sx[k4];
      if (next && c < d) {
        const double b = shi[c] + (-slo[c]);
        const double rc = (-sg[k4] * b) / m;
        x = x + ((tk * rc) * b);
        x = (x > slo[c]) ? x : slo[c];
        x = (x < shi[c]) ? x : shi[c];
      }
      xb[k4] = x;
    }
    if (rung == 0 && st < P && out.trace) {
      double *rec = out.trace + (((long long)j * TS_PMAX + st) * (iters + 1) + it) * B7_REFINE_TRACE_WIDTH;
#pragma unroll
      for (int k4 = 0; k4 < KS; ++k4) {
        const int c = 4 * k4 + lq;
        if (c < d) rec[c] = sx[k4], rec[d + 1 + c] = sg[k4];
      }
      if (lq == 0) {
        rec[d] = v;
        rec[2 * d + 1] = eta;
#pragma unroll
        for (int k = 0; k < 4; ++k) rec[2 * d + 2 + k] = cand[k];
        rec[2 * d + 6] = (it == 0) ? -1.0 : (double)taken;
        rec[2 * d + 7] = (double)status;
      }
    }
    eta = eta_new;
    active = next;
  }
  if (rung == 0 && st < P) {
    const long long e = (long long)j * TS_PMAX + st;
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) {
      const int c = 4 * k4 + lq;
      if (c < d) out.x[e * B7_MAX_D + c] = sx[k4], out.g[e * B7_MAX_D + c] = sg[k4];
    }
    if (lq == 0) out.v[e] = v, out.status[e] = status;
  }
}

// b7_ts_path_grad_at: block = (path blockIdx.x, 64 rows blockIdx.y), wave = 16 rows as its 16 columns
template <int KERN, int DPAD>
__global__ void __launch_bounds__(256) ts_path_grad_kernel(TsOps o, const double *__restrict__ X1, long long M1, int q, double *__restrict__ val,
                                                           double *__restrict__ grad) {
  constexpr int KS = DPAD / 4, NT = (DPAD + 15) / 16;
  __shared__ double stab[128], sw[DPAD], slo[DPAD], shi[DPAD];
  const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4, d = o.d;
  ts_tables<DPAD>(o, j, nullptr, stab, sw, slo, shi);
  const long long row = (long long)blockIdx.y * 64 + wave * 16 + lr;
  if ((long long)blockIdx.y * 64 + wave * 16 >= M1) return;  // wave-uniform
  double xb[KS];
#pragma unroll
  for (int k4 = 0; k4 < KS; ++k4) {
    const int c = 4 * k4 + lq;
    xb[k4] = (row < M1 && c < d) ? X1[row * d + c] : 0.0;
  }
  double v;
  d4_t G[NT];
  ts_eval16<KERN, DPAD>(o, j, stab, sw, xb, &v, G);
  if (row >= M1) return;
  if (lq == 0 && val) val[row * q + j] = v;
  if (grad)
#pragma unroll
    for (int k4 = 0; k4 < KS; ++k4) {
      const int c = 4 * k4 + lq;
      if (c < d) grad[(row * q + j) * d + c] = G[k4 >> 2][k4 & 3];
    }
}

// ---- the starts ---------------------------------------------------------------------------------------------------------------
// Path j's starts beyond its nominee: the n = starts - 1 rows of lowest f_j among the rows that are none of the q nominees,
// ascending by (value, row); a NaN is never chosen.  One pass over the paths: every workgroup leaves its slice's n lowest per path
// (the next one is the lowest above the previous: the order is total), one workgroup per path merges the lists the same way.
// (argbest.h: OrderMin, which is total only without NaNs -- a NaN value is skipped ahead of every comparison --, and block_best,
// which the loops below call again and again: a barrier ahead of every call frees its LDS slots)
__global__ void __launch_bounds__(256) ts_starts_kernel(const double *__restrict__ paths, long long M, int q, int n,
                                                        const long long *__restrict__ taken, ArgBest *__restrict__ part) {
  __shared__ ArgBest sh[4];
  const int j = blockIdx.y;
  long long tk[ARGBEST_MAX_EXCL];
  argbest_load_excl(taken, q, tk);
  ArgBest prev{0.0, -1};
  for (int p = 0; p < n; ++p) {
    ArgBest b{0.0, -1};
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < M; g += (long long)gridDim.x * 256) {
      const ArgBest cnd{paths[g * q + j], g};
      bool skip = cnd.v != cnd.v || argbest_excluded(tk, g);
      if (prev.i >= 0) skip = skip || !OrderMin()(prev, cnd);
      if (!skip && OrderMin()(cnd, b)) b = cnd;
    }
    __syncthreads();  // sh is free again
    b = block_best<OrderMin>(b, sh);
    if (threadIdx.x == 0) part[((long long)j * gridDim.x + blockIdx.x) * n + p] = b;
    prev = b;
    if (b.i < 0) {  // the slice is exhausted
      for (int r = p + 1 + threadIdx.x; r < n; r += 256) part[((long long)j * gridDim.x + blockIdx.x) * n + r] = ArgBest{0.0, -1};
      break;
    }
  }
}
// starts[j][0] = the nominee, starts[j][1 + p] = the p-th lowest of the partial lists (-1: none), starts[j][P ..] = -1
__global__ void __launch_bounds__(256) ts_starts_final_kernel(const ArgBest *__restrict__ part, int nblk, int n,
                                                              const long long *__restrict__ taken, long long *__restrict__ starts) {
  __shared__ ArgBest sh[4];
  const int j = blockIdx.x;
  const ArgBest *mine = part + (long long)j * nblk * n;
  if (threadIdx.x == 0) starts[j * TS_PMAX] = taken[j];
  ArgBest prev{0.0, -1};
  bool done = false;
  for (int p = 0; p < TS_PMAX - 1; ++p) {
    ArgBest b{0.0, -1};
    if (p < n && !done) {
      for (int e = threadIdx.x; e < nblk * n; e += 256) {
        const ArgBest c = mine[e];
        if (c.i < 0) continue;
        if (prev.i >= 0 && !OrderMin()(prev, c)) continue;
        if (OrderMin()(c, b)) b = c;
      }
      __syncthreads();  // sh is free again
      b = block_best<OrderMin>(b, sh);
      prev = b;
      done = b.i < 0;
    }
    if (threadIdx.x == 0) starts[j * TS_PMAX + 1 + p] = b.i;
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
struct TsRefWork {
  TsOps ops;
  double *hyp;        // [ns][d + 3]
  double *box;        // lo d | hi d
  long long *taken;   // [16]
  long long *starts;  // [q][16]
  ArgBest *part;       // [q][nblk][15]
  TsRefOut out;
  int nblk;
};

// the checks every entry shares: the kept paths are a GP's, of this grid and data
int ts_ref_check(b7_ctx *c, const char *who) {
  if (c->group) return b7_fail(c, B7_ERR_STATE, "%s: this context belongs to a group (sharded refinement of sample paths is not built)", who);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: a communicator of %d ranks (refinement of sample paths over a sharded grid is not built)", who,
                   c->comm_world);
  if (c->have_data && c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: %d response columns (one is built)", who, c->ycols);
  return B7_OK;
}
int ts_ref_kept(b7_ctx *c, const char *who, TsKept *k) {
  const int state = ts_state(c);
  if (state == TS_STATE_NONE) return b7_fail(c, B7_ERR_STATE, "%s: no successful b7_ts_nominate or b7_ts_paths on this context", who);
  if (state == TS_STATE_BLR)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the kept paths are the Bayesian-linear (DNGO) head's (their gradient is the basis network's Jacobian: not built)", who);
  if (state != TS_STATE_FRESH || ts_kept(c, k) != B7_OK)
    return b7_fail(c, B7_ERR_STATE, "%s: the kept paths are stale (the grid, the data or the covariance kernel changed since they were drawn)", who);
  return B7_OK;
}

// the operands of the kept paths into c->ts_ref_ws, in fragment order; the rest of the workspace carved behind them
int ts_ref_pack(b7_ctx *c, const TsKept &k, TsRefWork *wk) {
  const int q = c->ts.q, S = c->ts.S, F = c->ts.F, N = c->ts.N, d = c->ts.d, ns = k.ns;
  const int dpad = rff_dpad(d), NT = (dpad + 15) / 16, np16 = (int)round_up(N, 16);
  const int nblk = (int)std::min<int64_t>(512, (c->ts.M + 255) / 256);
  size_t off = 0;
  auto take = [&](size_t doubles) {
    const size_t o = off;
    off += (doubles + 31) / 32 * 32;
    return o;
  };
  const size_t o_omf = take((size_t)ns * F * dpad), o_omt = take((size_t)ns * F * 16 * NT), o_zf = take((size_t)ns * np16 * dpad);
  const size_t o_zt = take((size_t)ns * np16 * 16 * NT), o_zss = take((size_t)ns * np16), o_w = take((size_t)ns * dpad);
  const size_t o_Wp = take((size_t)q * F), o_vp = take((size_t)q * np16), o_par = take(2 * (size_t)q);
  const size_t o_hyp = take((size_t)ns * (d + 3)), o_box = take(2 * (size_t)d), o_taken = take(TS_PMAX), o_starts = take((size_t)q * TS_PMAX);
  const size_t o_part = take(2 * (size_t)q * nblk * (TS_PMAX - 1));
  const size_t o_x = take((size_t)q * TS_PMAX * B7_MAX_D), o_g = take((size_t)q * TS_PMAX * B7_MAX_D), o_v = take((size_t)q * TS_PMAX);
  const size_t o_st = take((size_t)q * TS_PMAX);
  B7_TRY(b7_ensure(c, c->ts_ref_ws, sizeof(double) * off));
  double *b = (double *)c->ts_ref_ws.p;
  TsOps &o = wk->ops;
  o.omf = b + o_omf, o.omt = b + o_omt, o.zf = b + o_zf, o.zt = b + o_zt, o.zss = b + o_zss, o.w = b + o_w;
  o.s_omf = (long long)F * dpad, o.s_omt = (long long)F * 16 * NT, o.s_zf = (long long)np16 * dpad, o.s_zt = (long long)np16 * 16 * NT;
  o.s_zss = np16;
  o.phase = k.phase, o.Wp = b + o_Wp, o.vp = b + o_vp, o.par = b + o_par;
  o.d = d, o.F = F, o.N = N, o.np16 = np16, o.S = S;
  wk->hyp = b + o_hyp, wk->box = b + o_box;
  wk->taken = reinterpret_cast<long long *>(b + o_taken), wk->starts = reinterpret_cast<long long *>(b + o_starts);
  wk->part = reinterpret_cast<ArgBest *>(b + o_part);
  wk->out.x = b + o_x, wk->out.g = b + o_g, wk->out.v = b + o_v, wk->out.status = reinterpret_cast<int *>(b + o_st), wk->out.trace = nullptr;
  wk->nblk = nblk;
  PhaseScope ps(c, "ts_refine:pack");
  B7_HIP(c, hipMemcpyAsync(wk->hyp, c->ts.hyp.data(), sizeof(double) * c->ts.hyp.size(), hipMemcpyHostToDevice, c->stream));
  const int64_t per = (int64_t)(F + np16) * (dpad + 16 * NT) + np16 + dpad;
  hipLaunchKernelGGL(ts_pack_sample_kernel, dim3((unsigned)std::min<int64_t>(1024, (per + 255) / 256), ns), dim3(256), 0, c->stream, k.omega,
                     (const double *)c->xobs.p, (const double *)wk->hyp, F, d, dpad, N, np16, b + o_omf, b + o_omt, b + o_zf, b + o_zt, b + o_zss,
                     b + o_w);
  hipLaunchKernelGGL(ts_pack_path_kernel, dim3((unsigned)((F + np16 + 2 + 255) / 256), q), dim3(256), 0, c->stream, k.weight, k.alpha,
                     (long long)k.alpha_stride, (const double *)wk->hyp, F, d, N, np16, S, q, b + o_Wp, b + o_vp, b + o_par);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

template <int KERN>
void ts_refine_launch(b7_ctx *c, const TsRefWork &wk, int q, int P, int iters, double eta0) {
  const double *grid = (const double *)c->grid[c->grid_cur].p;
#define B7_TS_REF_CASE(DP)                                                                                                        \
  hipLaunchKernelGGL((ts_refine_kernel<KERN, DP>), dim3(q), dim3(256), 0, c->stream, wk.ops, grid, (const long long *)wk.starts, \
                     (const double *)wk.box, P, iters, eta0, wk.out)
  switch (rff_dpad(wk.ops.d)) {
    case 8: B7_TS_REF_CASE(8); break;
    case 16: B7_TS_REF_CASE(16); break;
    case 32: B7_TS_REF_CASE(32); break;
    case 64: B7_TS_REF_CASE(64); break;
    default: B7_TS_REF_CASE(96); break;
  }
#undef B7_TS_REF_CASE
}

template <int KERN>
void ts_path_grad_launch(b7_ctx *c, const TsRefWork &wk, const double *X1, int64_t M1, int q, double *val, double *grad) {
#define B7_TS_GRAD_CASE(DP)                                                                                                      \
  hipLaunchKernelGGL((ts_path_grad_kernel<KERN, DP>), dim3(q, (unsigned)((M1 + 63) / 64)), dim3(256), 0, c->stream, wk.ops, X1, \
                     (long long)M1, q, val, grad)
  switch (rff_dpad(wk.ops.d)) {
    case 8: B7_TS_GRAD_CASE(8); break;
    case 16: B7_TS_GRAD_CASE(16); break;
    case 32: B7_TS_GRAD_CASE(32); break;
    case 64: B7_TS_GRAD_CASE(64); break;
    default: B7_TS_GRAD_CASE(96); break;
  }
#undef B7_TS_GRAD_CASE
}

}  // namespace

extern "C" {

int b7_ts_nominate_refine(b7_ctx *c, int S, const b7_hyp *hyps, int q, int F, uint64_t seed, const b7_refine_opts *opts, double *path_min,
                          int64_t *best_idx1, double *x_out, double *val_out, int64_t *start_idx1_out, double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  const char *who = "ts_nominate_refine";
  B7_TRY(ts_ref_check(c, who));
  if (!opts || !path_min || !best_idx1 || !x_out || !val_out || !start_idx1_out)
    return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (opts, path_min, best_idx1, x_out, val_out, start_idx1_out are required)", who);
  const int P = opts->starts, iters = opts->iters, d = c->dfit;
  if (P < 1 || P > B7_REFINE_MAX_STARTS || (c->M > 0 && P > c->M))
    return b7_fail(c, B7_ERR_INVALID, "%s: starts = %d not in [1, %d], or above the grid's %lld rows", who, P, B7_REFINE_MAX_STARTS, (long long)c->M);
  if (c->M > 0 && q >= 1 && q <= B7_BATCH_MAX && q <= c->M && P > c->M - q + 1)
    return b7_fail(c, B7_ERR_INVALID, "%s: starts = %d > M - q + 1 = %lld (a path's starts are its nominee and rows that are no path's nominee)", who, P,
                   (long long)(c->M - q + 1));
  if (iters < 0 || iters > B7_REFINE_MAX_ITERS) return b7_fail(c, B7_ERR_INVALID, "%s: iters = %d not in [0, %d]", who, iters, B7_REFINE_MAX_ITERS);
  if (!(opts->eta0 > 0.0 && opts->eta0 <= 1.0)) return b7_fail(c, B7_ERR_INVALID, "%s: eta0 = %g not in (0, 1]", who, opts->eta0);
  if ((opts->lo == nullptr) != (opts->hi == nullptr)) return b7_fail(c, B7_ERR_INVALID, "%s: lo and hi go together", who);
  std::vector<double> box(2 * (size_t)std::max(d, 1));
  for (int k = 0; k < d; ++k) {
    box[k] = opts->lo ? opts->lo[k] : 0.0, box[d + k] = opts->hi ? opts->hi[k] : 1.0;
    if (!std::isfinite(box[k]) || !std::isfinite(box[d + k]) || !(box[k] < box[d + k]))
      return b7_fail(c, B7_ERR_INVALID, "%s: box column %d is [%g, %g] (finite, lo < hi)", who, k, box[k], box[d + k]);
  }
  c->ts_ref_last.valid = false;
  // b7_ts_nominate's own checks, draws, fits, paths and arg-mins
  B7_TRY(b7_ts_nominate(c, S, hyps, q, F, seed, path_min, best_idx1, jitter_out, info_out));
  TsKept kept;
  B7_TRY(ts_ref_kept(c, who, &kept));
  TsRefWork wk;
  B7_TRY(ts_ref_pack(c, kept, &wk));
  long long tk[TS_PMAX];
  for (int j = 0; j < TS_PMAX; ++j) tk[j] = j < q ? (long long)best_idx1[j] - 1 : -1;
  B7_HIP(c, hipMemcpyAsync(wk.taken, tk, sizeof(tk), hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(wk.box, box.data(), sizeof(double) * 2 * d, hipMemcpyHostToDevice, c->stream));
  {
    PhaseScope ps(c, "ts_refine:starts");
    if (P > 1)
      hipLaunchKernelGGL(ts_starts_kernel, dim3(wk.nblk, q), dim3(256), 0, c->stream, (const double *)c->ts_paths.p, (long long)c->ts.M, q, P - 1,
                         (const long long *)wk.taken, wk.part);
    hipLaunchKernelGGL(ts_starts_final_kernel, dim3(q), dim3(256), 0, c->stream, (const ArgBest *)wk.part, wk.nblk, P - 1,
                       (const long long *)wk.taken, wk.starts);
    B7_HIP(c, hipGetLastError());
  }
  const bool traced = c->ts_ref_trace_on;
  if (traced) {
    const size_t tb = sizeof(double) * (size_t)q * TS_PMAX * (iters + 1) * B7_REFINE_TRACE_WIDTH;
    B7_TRY(b7_ensure(c, c->ts_ref_trace, tb));
    B7_HIP(c, hipMemsetAsync(c->ts_ref_trace.p, 0, tb, c->stream));
    wk.out.trace = (double *)c->ts_ref_trace.p;
  }
  {
    PhaseScope ps(c, "ts_refine");
    if (c->kernel == B7_KERNEL_MATERN52)
      ts_refine_launch<B7_KERNEL_MATERN52>(c, wk, q, P, iters, opts->eta0);
    else
      ts_refine_launch<B7_KERNEL_ARDSE>(c, wk, q, P, iters, opts->eta0);
    B7_HIP(c, hipGetLastError());
  }
  TsRefLast &last = c->ts_ref_last;
  std::vector<double> hx((size_t)q * TS_PMAX * B7_MAX_D);
  last.x.assign((size_t)q * TS_PMAX * d, 0.0), last.v.assign((size_t)q * TS_PMAX, NAN);
  last.idx.assign((size_t)q * TS_PMAX, -1), last.status.assign((size_t)q * TS_PMAX, B7_REFINE_NOT_RUN);
  B7_HIP(c, hipMemcpyAsync(hx.data(), wk.out.x, sizeof(double) * hx.size(), hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(last.v.data(), wk.out.v, sizeof(double) * last.v.size(), hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(last.idx.data(), wk.starts, sizeof(long long) * last.idx.size(), hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipMemcpyAsync(last.status.data(), wk.out.status, sizeof(int) * last.status.size(), hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < q * TS_PMAX; ++e) memcpy(&last.x[(size_t)e * d], &hx[(size_t)e * B7_MAX_D], sizeof(double) * d);
  // path j's winner: the lowest final value among the starts that ran, the lowest rank on ties; if none moved, the nominee
  for (int j = 0; j < q; ++j) {
    const int e0 = j * TS_PMAX;
    int win = 0;
    bool moved = false;
    for (int p = 0; p < P; ++p) moved = moved || (last.status[e0 + p] & B7_REFINE_MOVED);
    if (moved) {
      int best = -1;
      for (int p = 0; p < P; ++p) {
        if ((last.status[e0 + p] & B7_REFINE_NOT_RUN) || !std::isfinite(last.v[e0 + p])) continue;
        if (best < 0 || last.v[e0 + p] < last.v[e0 + best]) best = p;
      }
      if (best >= 0) win = best;
    }
    memcpy(x_out + (size_t)j * d, &last.x[(size_t)(e0 + win) * d], sizeof(double) * d);
    val_out[j] = last.v[e0 + win];
    start_idx1_out[j] = last.idx[e0 + win] + 1;
  }
  last.q = q, last.P = P, last.d = d, last.iters = iters, last.traced = traced, last.valid = true;
  return B7_OK;
}

int b7_ts_refine_last(b7_ctx *c, int path, int *P, double *x, double *val, int64_t *start_idx1, int *status) {
  if (!c) return B7_ERR_INVALID;
  const TsRefLast &last = c->ts_ref_last;
  if (!last.valid) return b7_fail(c, B7_ERR_STATE, "ts_refine_last: no successful b7_ts_nominate_refine on this context");
  if (path < 0 || path >= last.q) return b7_fail(c, B7_ERR_INVALID, "ts_refine_last: path %d not in [0, %d)", path, last.q);
  if (P) *P = last.P;
  for (int p = 0; p < last.P; ++p) {
    const size_t e = (size_t)path * TS_PMAX + p;
    if (x) memcpy(x + (size_t)p * last.d, &last.x[e * last.d], sizeof(double) * last.d);
    if (val) val[p] = last.v[e];
    if (start_idx1) start_idx1[p] = last.idx[e] + 1;
    if (status) status[p] = last.status[e];
  }
  return B7_OK;
}

int b7_ts_refine_trace_enable(b7_ctx *c, int on) {
  if (!c) return B7_ERR_INVALID;
  c->ts_ref_trace_on = on != 0;
  c->ts_ref_last.traced = false;
  return B7_OK;
}

int b7_ts_refine_trace(b7_ctx *c, int path, int start, double *records, int *n_records) {
  if (!c) return B7_ERR_INVALID;
  if (!n_records) return b7_fail(c, B7_ERR_INVALID, "ts_refine_trace: NULL argument");
  const TsRefLast &last = c->ts_ref_last;
  if (!last.valid || !last.traced)
    return b7_fail(c, B7_ERR_STATE, "ts_refine_trace: no traced b7_ts_nominate_refine (b7_ts_refine_trace_enable first)");
  if (path < 0 || path >= last.q || start < 0 || start >= last.P)
    return b7_fail(c, B7_ERR_INVALID, "ts_refine_trace: path %d of %d, start %d of %d", path, last.q, start, last.P);
  B7_HIP(c, hipSetDevice(c->device));
  const size_t per = (size_t)(last.iters + 1) * B7_REFINE_TRACE_WIDTH;
  if (records)
    B7_HIP(c, hipMemcpy(records, (const double *)c->ts_ref_trace.p + per * ((size_t)path * TS_PMAX + start), sizeof(double) * per,
                        hipMemcpyDeviceToHost));
  *n_records = last.iters + 1;
  return B7_OK;
}

int b7_ts_path_grad_at(b7_ctx *c, const double *X1, int64_t M1, double *val, double *grad) {
  if (!c) return B7_ERR_INVALID;
  const char *who = "ts_path_grad_at";
  B7_TRY(ts_ref_check(c, who));
  if (M1 < 0 || (!X1 && M1 > 0)) return b7_fail(c, B7_ERR_INVALID, "%s: bad X1/M1", who);
  TsKept kept;
  B7_TRY(ts_ref_kept(c, who, &kept));
  if (M1 == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const int q = c->ts.q, d = c->ts.d;
  TsRefWork wk;
  B7_TRY(ts_ref_pack(c, kept, &wk));
  const size_t nx = (size_t)M1 * d, nv = (size_t)M1 * q, ng = nv * d;
  B7_TRY(b7_ensure(c, c->ts_ref_user, sizeof(double) * (nx + nv + ng)));
  double *Xd = (double *)c->ts_ref_user.p, *vd = Xd + nx, *gd = vd + nv;
  B7_HIP(c, hipMemcpyAsync(Xd, X1, sizeof(double) * nx, hipMemcpyHostToDevice, c->stream));
  {
    PhaseScope ps(c, "ts_refine:grad_at");
    if (c->kernel == B7_KERNEL_MATERN52)
      ts_path_grad_launch<B7_KERNEL_MATERN52>(c, wk, Xd, M1, q, vd, gd);
    else
      ts_path_grad_launch<B7_KERNEL_ARDSE>(c, wk, Xd, M1, q, vd, gd);
    B7_HIP(c, hipGetLastError());
  }
  if (val) B7_HIP(c, hipMemcpyAsync(val, vd, sizeof(double) * nv, hipMemcpyDeviceToHost, c->stream));
  if (grad) B7_HIP(c, hipMemcpyAsync(grad, gd, sizeof(double) * ng, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

}  // extern "C"

// Thompson sampling for the Bayesian-linear head (DNGO) -- b7_blr_ts_nominate, b7_blr_ts_last_draws, b7_blr_paths_compute.
//
// No counterpart in the reference.  The head's posterior over its weights is a finite Gaussian, w ~ N(m_s, inv(A_s)) with
// A_s = alpha_s I + beta_s Z'Z = L_s L_s', so a sample path is exact and needs neither random features nor a pseudo-response fit:
//   f_j(x) = mean_s + phi(x)' w_j,      w_j = m_s + L_s^-T eps_j,      eps_j ~ N(0, I_z),      s = j mod S
// (the covariance of L^-T eps is L^-T L^-1 = inv(A); L^-1 eps would have L^-1 L^-T, which is NOT inv(A)).  Paths are of the latent
// function: the 1 / beta observation noise is not added, exactly as the GP's paths carry none.
//
// The fits and the candidates' features are b7_blr_eval_nominate_marg's (blr_api.hip: one basis pass over the observations, the S
// heads side by side in one launch for z <= 64 or head by head through b7_blr_fit_x, one basis pass over the resident grid), the
// arg-mins are rff.hip's.  New here:
//
// blr_ts_weights_kernel, one workgroup per path.  eps_j[k] = counter_normal(key(seed, 2^32 + j), k) (counter_rng.h: a stream of its
// own; rff.hip's are 0 and 1 + j); w_j[k] = m_s[k] + a_k, a_k = sum_{i >= k} L^-1[i][k] eps_j[i] as ONE fma chain from 0 over
// ascending i, then one addition.  It leaves eps and w for b7_blr_ts_last_draws, w once more in the order the paths kernel reads
// (frag_index below), and mean0[j] = mean_s.
//
// blr_paths_kernel<ZPAD>:  out[i][j] = mean0[j] + sum_k feat[i][k] W[k][j],   i < M, j < q <= 16, k < ZPAD in {64, 128, 256}
// on v_mfma_f64_16x16x4 (gemm_f64.h's maps), the 16 candidates of a tile as the A operand's rows and the q <= 16 paths, padded with
// zero columns to exactly one tile, as the B operand's columns.  Per tile a lane reads 16 bytes at (row lane & 15, column
// 16 c + 8 h + 2 (lane >> 4)) for c < ZPAD / 16, h < 2: every load instruction takes 64 contiguous bytes of each of 16 rows, a pair
// of them whole 128-byte lines, and the resident feature buffer is read exactly once.
//   THE K ORDER, the same whatever M and q are: chunks of 16 columns in ascending order c; within a chunk four MFMA steps t = 0 .. 3,
//   step t taking the columns 16 c + 8 (t >> 1) + (t & 1) + {0, 2, 4, 6} (one per lane group, summed by the instruction onto the
//   running accumulator, which starts at +0.0).  mean0[j] is added ONCE, after the last chunk: out = mean0[j] + acc, one rounding.
//   An element's bits therefore depend on its own feature row and its own weight column alone: not on M, not on q, not on the other
//   columns (a column of the tile is its own dot product), not on ZPAD beyond z (the padding of both operands is +0.0).
//   A NaN feature row gives a NaN output row and touches no other row; rows beyond M are staged as zeros.
// W staging: LDS, once per workgroup, already in fragment order so that a step's operand is one conflict-free ds_read_b64 per
// lane.  Registers would hold ZPAD / 4 doubles per lane (128 VGPRs at ZPAD = 256) beside the features in flight, and this kernel
// lives on loads in flight: it is bound by the feature read, M ZPAD 8 bytes, plus M q 8 written; its ZPAD / 4 MFMAs per tile of 16
// rows (64 cycles each, 1024 SIMDs) keep pace with about three times the memory's rate.  Each wave walks tiles with a grid stride
// and takes a tile 64 columns at a time; there is no pipelining beyond the waves in flight (4 to 6 per SIMD).
//
// Out of scope: sharded grids and groups, the kept posterior / EHVI / constraints for this head, and fusing the product into the
// basis kernel's epilogue so that the features are never stored (the obvious next lever).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"
#include "counter_rng.h"
#include "gemm_f64.h"

namespace {

constexpr uint64_t BLR_TS_STREAM = 1ull << 32;  // path j draws from key(seed, 2^32 + j)

// where W[k][col] sits in the fragment-ordered image (zpad x 16 doubles): step (c, t) is 64 consecutive doubles, one per lane
__host__ __device__ inline int frag_index(int k, int col) {
  const int c = k >> 4, r = k & 15, t = 2 * (r >> 3) + (r & 1), lq = (r & 7) >> 1;
  return (c * 4 + t) * 64 + lq * 16 + col;
}

// Path j = j0 + blockIdx.x jstride under head s = j mod S: Linv + s sLinv (row stride ld), m + s sm; mean_dev[s] (or mean_host when
// mean_dev is null) -> mean0[j].  eps_out, w_out: [q][z]; wfrag: the zeroed fragment image, of which this block writes column j.
__global__ void __launch_bounds__(256) blr_ts_weights_kernel(uint64_t seed, int j0, int jstride, int S, const double *__restrict__ Linv,
                                                             int64_t sLinv, int ld, const double *__restrict__ m, int64_t sm,
                                                             const double *__restrict__ mean_dev, double mean_host, int z, int zpad,
                                                             double *__restrict__ eps_out, double *__restrict__ w_out,
                                                             double *__restrict__ wfrag, double *__restrict__ mean0) {
  __shared__ double e[256];
  const int j = j0 + blockIdx.x * jstride, s = j % S, k = threadIdx.x;
  const uint64_t key = counter_key(seed, BLR_TS_STREAM + (uint64_t)j);
  e[k] = k < z ? counter_normal(key, (uint64_t)k) : 0.0;
  __syncthreads();
  Linv += s * sLinv;
  m += s * sm;
  double w = 0.0;
  if (k < z) {
    double a = 0.0;
    for (int i = k; i < z; ++i) a = __builtin_fma(Linv[(int64_t)i * ld + k], e[i], a);
    w = m[k] + a;
    eps_out[(int64_t)j * z + k] = e[k];
    w_out[(int64_t)j * z + k] = w;
  }
  if (k < zpad) wfrag[frag_index(k, j)] = w;
  if (k == 0) mean0[j] = mean_dev ? mean_dev[s] : mean_host;
}

template <int ZPAD>
__global__ void __launch_bounds__(256) blr_paths_kernel(const double *__restrict__ feat, int64_t M, const double *__restrict__ wfrag,
                                                        const double *__restrict__ mean0, int q, double *__restrict__ out) {
  constexpr int NC = ZPAD / 16;
  __shared__ double wsm[ZPAD * 16];
  for (int e = threadIdx.x; e < ZPAD * 16; e += 256) wsm[e] = wfrag[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const double mj = lr < q ? mean0[lr] : 0.0;
  const int64_t ntile = (M + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntile; tile += (int64_t)gridDim.x * 4) {
    const int64_t g = tile * 16 + lr;
    const bool live = g < M;
    const double *src = feat + (live ? g : 0) * ZPAD + 2 * lq;
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    // 64 columns (four chunks) at a time, not unrolled beyond that: 32 registers of features in flight per lane whatever ZPAD is,
    // and W's fragments stay in LDS (unrolled, the compiler keeps all of them in registers: one wave per SIMD at ZPAD = 256)
#pragma unroll 1
    for (int c0 = 0; c0 < NC; c0 += 4) {
      d2_t f[4][2];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) f[c][h] = live ? *reinterpret_cast<const d2_t *>(src + 16 * (c0 + c) + 8 * h) : d2_t{0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = mfma_f64(f[c][t >> 1][t & 1], wsm[((c0 + c) * 4 + t) * 64 + lane], acc);
    }
    // acc[r]: candidate tile 16 + lq + 4 r, path lr
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = tile * 16 + lq + 4 * r;
      if (row < M && lr < q) out[row * q + lr] = mj + acc[r];
    }
  }
}

// c->ts_work for a call of q paths over M rows: wfrag zpad x 16 | mean0 16 | pmin q | taken q | part 2 nblk, each piece on a
// 256-byte boundary
void blr_ts_work_layout(int zpad, int q, int nblk, size_t off[6]) {
  const size_t pieces[5] = {16 * (size_t)zpad, (size_t)B7_BATCH_MAX, (size_t)q, (size_t)q, 2 * (size_t)nblk};
  off[0] = 0;
  for (int i = 0; i < 5; ++i) off[i + 1] = off[i] + (size_t)round_up((int64_t)pieces[i], 32);
}

int launch_blr_ts_weights(b7_ctx *c, uint64_t seed, int j0, int jstride, int count, int S, const double *Linv, int64_t sLinv, int ld,
                          const double *m, int64_t sm, const double *mean_dev, double mean_host, int z, int zpad, double *eps_out,
                          double *w_out, double *wfrag, double *mean0) {
  PhaseScope ps(c, "blr_ts_weights");
  if (count <= 0) return B7_OK;
  hipLaunchKernelGGL(blr_ts_weights_kernel, dim3(count), dim3(256), 0, c->stream, seed, j0, jstride, S, Linv, sLinv, ld, m, sm, mean_dev,
                     mean_host, z, zpad, eps_out, w_out, wfrag, mean0);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// feat: M rows of zpad doubles (zero beyond the head's z columns); wfrag, mean0 as blr_ts_weights_kernel leaves them; out: M x q
int launch_blr_paths(b7_ctx *c, const double *feat, int64_t M, int zpad, const double *wfrag, const double *mean0, int q, double *out) {
  PhaseScope ps(c, "blr_paths");
  if (M <= 0) return B7_OK;
  const int64_t ntile = (M + 15) / 16;
  const dim3 grid((unsigned)std::min<int64_t>((ntile + 3) / 4, 2048)), block(256);
  switch (zpad) {
    case 64: hipLaunchKernelGGL(blr_paths_kernel<64>, grid, block, 0, c->stream, feat, M, wfrag, mean0, q, out); break;
    case 128: hipLaunchKernelGGL(blr_paths_kernel<128>, grid, block, 0, c->stream, feat, M, wfrag, mean0, q, out); break;
    case 256: hipLaunchKernelGGL(blr_paths_kernel<256>, grid, block, 0, c->stream, feat, M, wfrag, mean0, q, out); break;
    default: return b7_fail(c, B7_ERR_UNSUPPORTED, "blr_paths: padded basis width %d (64, 128 and 256 are built)", zpad);
  }
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// the S heads head by head through b7_blr_fit_x (synchronous, jitter schedule included); the weights of head s's paths follow its fit
int blr_ts_heads_slow(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap, const double *bt,
                      const double *mn, int q, uint64_t seed, int z, int zpad, double *eps, double *weight, double *wfrag, double *mean0,
                      double *nll_out) {
  for (int s = 0; s < S; ++s) {
    B7_TRY(b7_blr_fit_x(c, net, X0, Y0, N, ap[s], bt[s], mn[s], nll_out ? nll_out + s : nullptr));
    if (s < q)
      B7_TRY(launch_blr_ts_weights(c, seed, s, S, (q - s + S - 1) / S, S, (const double *)c->Linv.p, 0, c->Npad, (const double *)c->alpha.p, 0,
                                   nullptr, mn[s], z, zpad, eps, weight, wfrag, mean0));
  }
  return B7_OK;
}

}  // namespace

extern "C" {

int b7_blr_ts_nominate(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap, const double *bt,
                       const double *mn, int q, uint64_t seed, double *path_min, int64_t *best_idx1, double *nll_out, double *jitter_used) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "blr_ts_nominate: this context belongs to a group (sharded Thompson sampling is not built)");
  if (jitter_used) *jitter_used = 0.0;
  if (q < 1 || q > B7_BATCH_MAX) return b7_fail(c, B7_ERR_INVALID, "blr_ts_nominate: q = %d not in [1, %d]", q, B7_BATCH_MAX);
  if (S < 1) return b7_fail(c, B7_ERR_INVALID, "blr_ts_nominate: S = %d hyper samples (at least one)", S);
  if (!net || !X0 || !Y0 || N < 1 || !ap || !bt || !mn || !path_min || !best_idx1)
    return b7_fail(c, B7_ERR_INVALID, "blr_ts_nominate: NULL argument (net, X0, Y0, the S hypers, path_min and best_idx1 are needed) or N < 1");
  for (int s = 0; s < S; ++s)
    if (!(ap[s] > 0.0) || !(bt[s] > 0.0)) return b7_fail(c, B7_ERR_INVALID, "blr_ts_nominate: precisions must be > 0 (sample %d)", s);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "blr_ts_nominate: a communicator of %d ranks (sharded Thompson sampling is not built)", c->comm_world);
  if (c->M <= 0 || c->d <= 0) return b7_fail(c, B7_ERR_STATE, "blr_ts_nominate: no candidate grid on this context");
  if (q > c->M) return b7_fail(c, B7_ERR_INVALID, "blr_ts_nominate: q = %d exceeds the grid's %lld rows", q, (long long)c->M);
  B7_HIP(c, hipSetDevice(c->device));
  int z = 0;
  B7_TRY(blr_upload_net(c, net, &z));
  if (z > 256) return b7_fail(c, B7_ERR_UNSUPPORTED, "blr: basis width %d > 256", z);
  if (net->dims[0] != c->d) return b7_fail(c, B7_ERR_INVALID, "blr_ts_nominate: network input width %d != grid dims %d", net->dims[0], c->d);
  const int64_t M = c->M;
  const int zpad = npad_of(c, z), nblk = argbest_blocks(M);
  TsPaths &kept = c->ts;
  kept.who = TS_NONE;

  B7_TRY(b7_ensure(c, c->ts_paths, sizeof(double) * (size_t)M * q));
  B7_TRY(b7_ensure(c, c->ts_draw, sizeof(double) * 2 * (size_t)q * z));  // eps [q][z] | weight [q][z]
  size_t off[6];
  blr_ts_work_layout(zpad, q, nblk, off);
  B7_TRY(b7_ensure(c, c->ts_work, sizeof(double) * off[5]));
  double *eps = (double *)c->ts_draw.p, *weight = eps + (size_t)q * z;
  double *wk = (double *)c->ts_work.p, *wfrag = wk + off[0], *mean0 = wk + off[1], *pmin = wk + off[2];
  long long *taken = reinterpret_cast<long long *>(wk + off[3]);
  double *paths = (double *)c->ts_paths.p;
  long long tk[B7_BATCH_MAX];

  // the candidates' features, the paths and the arg-mins behind whatever produced the weights; waits for the stream
  auto tail = [&]() -> int {
    B7_TRY(blr_feat_alloc(c, M, z));
    B7_TRY(launch_mlp_forward(c, (const double *)c->grid[c->grid_cur].p, M, c->d, (const double *)c->netbuf.p, net->dims, net->n_layers,
                              net->activation, (double *)c->feat.p, zpad));
    B7_TRY(launch_blr_paths(c, (const double *)c->feat.p, M, zpad, wfrag, mean0, q, paths));
    B7_TRY(launch_ts_argmins(c, paths, M, q, pmin, taken, reinterpret_cast<ArgBest *>(wk + off[4]), nblk));
    B7_HIP(c, hipMemcpyAsync(path_min, pmin, sizeof(double) * q, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipMemcpyAsync(tk, taken, sizeof(long long) * q, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    return B7_OK;
  };

  bool by_head = !(z <= 64 && c->blr_small && c->npad_small);
  if (!by_head) {
    // z <= 64: nothing waits for the host until the nominees are out -- the S heads in one launch, the q weight columns from their
    // factors, the features, the paths, the arg-mins; the pivot reports are read afterwards
    double *hdev = nullptr;
    B7_TRY(blr_heads_fast_enqueue(c, net, X0, Y0, N, S, ap, bt, mn, z, nll_out != nullptr, &hdev));
    B7_HIP(c, hipMemsetAsync(wfrag, 0, sizeof(double) * 16 * (size_t)zpad, c->stream));
    B7_TRY(launch_blr_ts_weights(c, seed, 0, 1, q, S, (const double *)c->bLinv.p, 64 * 64, 64, (const double *)c->balpha.p, 64,
                                 hdev + 2 * (size_t)S, 0.0, z, zpad, eps, weight, wfrag, mean0));
    B7_TRY(tail());
    if (reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, false)) {
      if (nll_out) {  // the evidence of every head from the kernel's three sums, as b7_blr_eval_nominate_marg forms it
        const double *t = reinterpret_cast<const double *>(static_cast<const char *>(c->pin_eval.host) + 16 * (size_t)S);
        for (int s = 0; s < S; ++s) {
          const double Em = 0.5 * bt[s] * t[3 * s + 2] - 0.5 * t[3 * s + 1];
          nll_out[s] = -(0.5 * z * log(ap[s]) + 0.5 * N * log(bt[s]) - Em - t[3 * s] - 0.5 * N * log(2.0 * M_PI));
        }
      }
      c->fitted = false;  // the context's own fit slot holds none of the S heads
    } else {
      by_head = true;  // a failed pivot: the heads again through the jitter schedule, and the paths from the jittered factors
      if (jitter_used) *jitter_used = -2.0;
    }
  }
  if (by_head) {
    B7_HIP(c, hipMemsetAsync(wfrag, 0, sizeof(double) * 16 * (size_t)zpad, c->stream));
    B7_TRY(blr_ts_heads_slow(c, net, X0, Y0, N, S, ap, bt, mn, q, seed, z, zpad, eps, weight, wfrag, mean0, nll_out));
    B7_TRY(tail());
  }
  for (int j = 0; j < q; ++j) best_idx1[j] = tk[j] + 1;
  kept.M = M, kept.q = q, kept.S = S, kept.F = z, kept.N = 0, kept.d = 0, kept.ns = S < q ? S : q;
  kept.epoch = c->epoch;
  kept.alpha = nullptr, kept.alpha_stride = 0;
  kept.pmin = pmin, kept.taken = taken, kept.part = reinterpret_cast<ArgBest *>(wk + off[4]), kept.nblk = nblk;
  kept.who = TS_BLR;
  return B7_OK;
}

int b7_blr_ts_last_draws(b7_ctx *c, int path, double *eps, double *weight) {
  if (!c) return B7_ERR_INVALID;
  if (ts_state(c) != TS_STATE_BLR) return b7_fail(c, B7_ERR_STATE, "blr_ts_last_draws: no successful b7_blr_ts_nominate on this context");
  if (path < 0 || path >= c->ts.q) return b7_fail(c, B7_ERR_INVALID, "blr_ts_last_draws: path %d not in [0, %d)", path, c->ts.q);
  B7_HIP(c, hipSetDevice(c->device));
  const int z = c->ts.F, q = c->ts.q;
  const double *e = (const double *)c->ts_draw.p, *w = e + (size_t)q * z;
  if (eps) B7_HIP(c, hipMemcpyAsync(eps, e + (size_t)path * z, sizeof(double) * z, hipMemcpyDeviceToHost, c->stream));
  if (weight) B7_HIP(c, hipMemcpyAsync(weight, w + (size_t)path * z, sizeof(double) * z, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_blr_paths_compute(b7_ctx *c, const double *Z, int64_t M1, int z, const double *W, const double *mean0, int q, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (!Z || !W || !mean0 || !out) return b7_fail(c, B7_ERR_INVALID, "blr_paths_compute: NULL argument");
  if (M1 < 1 || z < 1 || z > 256) return b7_fail(c, B7_ERR_INVALID, "blr_paths_compute: M1 = %lld rows, z = %d (1..256)", (long long)M1, z);
  if (q < 1 || q > B7_BATCH_MAX) return b7_fail(c, B7_ERR_INVALID, "blr_paths_compute: q = %d not in [1, %d]", q, B7_BATCH_MAX);
  B7_HIP(c, hipSetDevice(c->device));
  const int zpad = npad_of(c, z);
  // Z M1 zpad (zero padded) | out M1 q | wfrag 16 zpad | mean0 16 -- a buffer of its own: the last nomination's paths and draws stay
  const size_t nz = (size_t)M1 * zpad, no = (size_t)round_up(M1 * q, 2), nw = 16 * (size_t)zpad;
  B7_TRY(b7_ensure(c, c->ts_user, sizeof(double) * (nz + no + nw + B7_BATCH_MAX)));
  double *Zd = (double *)c->ts_user.p, *od = Zd + nz, *wd = od + no, *md = wd + nw;
  std::vector<double> stage(nw + B7_BATCH_MAX, 0.0);  // W in fragment order (a layout change, no arithmetic) | mean0
  for (int k = 0; k < z; ++k)
    for (int j = 0; j < q; ++j) stage[frag_index(k, j)] = W[(size_t)k * q + j];
  memcpy(&stage[nw], mean0, sizeof(double) * q);
  if (zpad != z) B7_HIP(c, hipMemsetAsync(Zd, 0, sizeof(double) * nz, c->stream));
  B7_HIP(c, hipMemcpy2DAsync(Zd, sizeof(double) * zpad, Z, sizeof(double) * z, sizeof(double) * z, M1, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(wd, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_blr_paths(c, Zd, M1, zpad, wd, md, q, od));
  B7_HIP(c, hipMemcpyAsync(out, od, sizeof(double) * (size_t)M1 * q, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staging vector are consumed
  return B7_OK;
}

}  // extern "C"

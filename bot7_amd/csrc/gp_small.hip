// The GP fit for SMALL observation sets -- N <= 128, d <= 32, one response column: the reference's own regime (budget 100,
// bots/abstract.lua:64) -- in ONE workgroup of ONE launch per hyper vector.
//
// Reference arithmetic replaced, per hyper vector (bots/bayesopt.lua:68,73-76 -> model:sample_hypers / model:predict's first half):
//   K(X,X) + noise I (utils/math.lua:65-111), chol (utils/math.lua:159-218: the plain attempt; a failed pivot is reported and
//   the caller redoes that fit through the general path and its jitter schedule), and then either
//     MODE 0  the likelihood's two reductions, |L^-1 r|^2 and sum log L_ii  (one density evaluation of samplers/slice.lua:92-168)
//     MODE 1  L^-1 in full, alpha = L^-T L^-1 r and the scaled observations: everything the posterior kernels read
//             (b7_eval_nominate's S fits are S workgroups of one launch: observation scaling, K(X,X), its fix-up, two memsets,
//             the persistent factorisation and three triangular matrix-vector launches of the general schedule in one).
//
// Structure.  512 threads.  Waves 0..3 are the four waves b7diag::diag_core is written for; waves 4..7 keep in step with its
// barriers (diag_bystander).  While wave 0 runs block (0,0)'s four pivot chains, everybody who is idle -- waves 4..7, and waves
// 1..3 through the routine's hook -- assembles what does not depend on L11: the rest of K11, all of K21, the K entries of
// block (1,1) (kept in LDS until L21 L21' is there to be subtracted); while it runs block (1,1)'s, waves 4..7 do the
// likelihood's first solve and the update of the second residual.  Four 64 x 66 images in LDS change roles as the data die:
// B0 observations -> inv(L22);  B1 K11 / L11 -> K22 / L22;  B2 K21 -> L21 -> L21 inv(L11) -> inv(L)21;  B3 inv(L11).
// The kernel is latency all the way: ONE workgroup executes ~40 KB of straight-line code once, out of an instruction cache that
// is cold at every launch (a sub-tile's code costs 2 300 cycles the first time and 1 700 the second) -- hence one instance per
// block count (TWO) and one site of sub-tile code per caller (k_job) rather than one per use.
//
// Bits.  K entries: the chain of v_mfma_f64_16x16x4 over the input dimensions, the (c - xs/2) - zs/2 argument and the table
// exponential of ksx_kernel (ksx_exp.h).  L, L^-1: diag_core per 64-block; L21 = C inv(L11)' with the blocks above inv(L11)'s
// diagonal skipped; K22 - L21 L21' as the 64-deep chain from zero, then the subtraction (lower sub-tiles only);
// inv(L)21 = -inv(L22) (0 + L21 inv(L11)) with the two alternating accumulators of potrf_persist.hip's inv_job -- the
// persistent schedule's arithmetic, operation for operation.  alpha: the sums of trmv_lower_kernel / trmv_lower_t_part_kernel
// (two 64-block systems) or of potrf_small64_kernel (one).  tests/test_gpu_parity.py holds L, L^-1 and alpha against the
// general path BIT FOR BIT and the likelihood against nll_small_kernel's bits.
#include "b7_internal.h"
#include "ksx_exp.h"
#include "potrf_diag.h"

#ifdef B7_GS_STAMP
// Diagnostic build only (tools/gp_small_stamps.py; never defined for the shipped library): workgroup 0's waves 0 and 4 record
// s_memtime at their phase boundaries into a buffer nothing else reads.
__device__ unsigned long long b7_gs_stamps[2 * 32 + 32];
extern "C" int b7dbg_gs_stamps(unsigned long long *out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(b7_gs_stamps), sizeof(unsigned long long) * (2 * 32 + 32));
}
#define GS_STAMP(i)                                                                                          \
  if (blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == 256)) b7_gs_stamps[(threadIdx.x >> 8) * 32 + (i)] = __builtin_amdgcn_s_memtime()
#else
#define GS_STAMP(i)
#endif

#include "gp_small_body.h"

namespace {
template <int MODE, bool TWO, int KERN>
__global__ void __launch_bounds__(GS_THREADS) gp_small_kernel(GsArgs a, GsInline hin) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int d = a.d, B = a.B;
  const double *hyp = a.use_inline ? hin.v : a.hyp_mem;
  const double *ls = hyp + (size_t)b * d;
  const double amp = hyp[(size_t)B * d + b], noise = hyp[(size_t)B * (d + 1) + b], mean = hyp[(size_t)B * (d + 2) + b];
  double t0 = 0.0, t1 = 0.0;
  int *inf;
  gs_body<MODE, TWO, KERN>(a, b, ls, amp, noise, mean, t0, t1, inf);
  if (MODE == 0 && tid == 0) {
    a.terms[2 * b] = t0;
    a.terms[2 * b + 1] = t1;
  }
  if (tid == 0) {
    if (a.info)
      for (int k = 0; k < 4; ++k) a.info[4 * b + k] = inf[k];
    if (a.report)
      for (int k = 0; k < 4; ++k) a.report[4 * b + k] = inf[k];
  }
  if (a.done) {
    // a single evaluation's caller spins on this word instead of waiting for the dispatch to retire (MODE 0: thread 0 wrote
    // everything the host reads; the release orders it before the flag as the host sees them)
    if (tid == 0) __hip_atomic_store(a.done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <int MODE, bool TWO, int KERN>
int gs_launch2(b7_ctx *c, const GsArgs &a, const double *hyp_host) {
  const size_t lds = sizeof(double) * GS_LDS_DOUBLES;
  // the opt-in to > 64 KiB of dynamic LDS is per device: once per process AND device (a process may hold contexts on several)
  static bool attr_done[64] = {false};
  if (c->device >= 64 || !attr_done[c->device]) {
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(gp_small_kernel<MODE, TWO, KERN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (c->device < 64) attr_done[c->device] = true;
  }
  GsInline hin = {};
  GsArgs k = a;
  k.use_inline = (a.B == 1 && hyp_host != nullptr) ? 1 : 0;
  for (int i = 0; k.use_inline && i < a.d + 3; ++i) hin.v[i] = hyp_host[i];
  hipLaunchKernelGGL((gp_small_kernel<MODE, TWO, KERN>), dim3(a.B), dim3(GS_THREADS), lds, c->stream, k, hin);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}
template <int MODE, int KERN>
int gs_launch_k(b7_ctx *c, const GsArgs &a, const double *hyp_host) {
  return a.N > NB ? gs_launch2<MODE, true, KERN>(c, a, hyp_host) : gs_launch2<MODE, false, KERN>(c, a, hyp_host);
}
template <int MODE>
int gs_launch(b7_ctx *c, const GsArgs &a, const double *hyp_host) {
  return c->kernel == B7_KERNEL_MATERN52 ? gs_launch_k<MODE, B7_KERNEL_MATERN52>(c, a, hyp_host)
                                         : gs_launch_k<MODE, B7_KERNEL_ARDSE>(c, a, hyp_host);
}

}  // namespace

// (the kernel pads N to one or two 64-blocks itself; a context told to pad small sets to 128 -- the diagnostic build's
// B7_NPAD_SMALL=0 -- keeps the general path)
bool gp_small_applies(const b7_ctx *c) { return c->Npad == (c->N > 64 ? 128 : 64) && c->dfit <= 32 && c->ycols == 1; }

// B likelihood evaluations of the resident data.  hyp_dev: [B x d lengthscales | B amp | B noise | B mean] (b7_gp_nll_batch's
// pack, device-visible); terms_dev[2 B], info_dev[4 B]; done_dev (nullable): a word the kernel sets to 1 after its results
// are visible to the host (B == 1 only).  hyp_host: the same pack in host memory; a single evaluation's hypers travel in the
// kernel arguments instead.
int launch_nll_small8(b7_ctx *c, int B, const double *hyp_dev, const double *hyp_host, double *terms_dev, int *info_dev,
                      unsigned *done_dev) {
  PhaseScope ps(c, "potrf");
  GsArgs a = {};
  a.xobs = (const double *)c->xobs.p;
  a.y = (const double *)c->ybuf.p;
  a.N = c->N, a.d = c->dfit, a.dpad = c->dpad, a.B = B;
  a.hyp_mem = hyp_dev;
  a.info = info_dev;
  a.done = B == 1 ? done_dev : nullptr;
  a.terms = terms_dev;
  return gs_launch<0>(c, a, hyp_host);
}

// B whole fits of the resident data (b7_eval_nominate's hyper samples; B = 1: the context's own fit slot).  The outputs are laid
// out as the general path's batch buffers: w [B][dpad], zsc [B][Npad][dpad], zss [B][Npad], Linv (and L, nullable) [B][Npad^2],
// dinv (nullable) [B][Npad 64], alpha (and resid, nullable) [B][Npad]; hyp_out (nullable) receives the pack for the kernels
// downstream.  info_dev / report_dev: 4 ints per fit, the second in mapped host memory (either may be null).
int launch_fit_small(b7_ctx *c, int B, const double *hyp_dev, const double *hyp_host, double *hyp_out, double *w, double *zsc,
                     double *zss, double *L, double *Linv, double *dinv, double *alpha, double *resid, int *info_dev,
                     int *report_dev) {
  PhaseScope ps(c, "potrf");
  GsArgs a = {};
  a.xobs = (const double *)c->xobs.p;
  a.y = (const double *)c->ybuf.p;
  a.N = c->N, a.d = c->dfit, a.dpad = c->dpad, a.B = B;
  a.hyp_mem = hyp_dev;
  a.info = info_dev;
  a.report = report_dev;
  a.hyp_out = hyp_out;
  a.w = w, a.zsc = zsc, a.zss = zss, a.L = L, a.Linv = Linv, a.dinv = dinv, a.alpha = alpha, a.resid = resid;
  return gs_launch<1>(c, a, hyp_host);
}

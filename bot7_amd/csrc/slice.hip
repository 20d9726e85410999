// b7_gp_slice_sample: the slice sampler's hyper chain (samplers/slice.lua:51-168, the default mode) on the device -- C chains of
// U updates in ONE launch of slice_chain_kernel (the sampler's control flow and the likelihood body of gp_small_body.h loop
// inside the kernel), one wait on a completion counter.  Below the kernel: argument checks, the pinned mapped block the kernel
// reads its start points from and writes its samples into, the wait, and the trace's read-back.
// This file is built with machine-level loop-invariant code motion off (build.py): with it, the address arithmetic and the
// constants of the 40 KB likelihood body are all formed ahead of the evaluation loop and kept there, which the body's own
// register needs turn into scratch traffic.
#include "gp_small_body.h"
#include "counter_rng.h"

#include <chrono>
#include <cmath>
#include <cstring>

namespace {
struct SliceArgs {
  int D, U, max_step, max_evals;               // D = d + 3 components of theta
  unsigned long long seed, update0;
  double c0;                                   // 0.5 N log(2 pi)
  const double *theta0, *lo, *hi, *widths;     // [C][D], [D], [D], [D]: device-visible (the mapped block)
  double *theta_out, *value_out;               // [C][U][D], [C][U]: mapped host memory
  int *status_out, *nevals_out;                // [C][U], [C]
  unsigned *done;                              // completion counter in mapped host memory: every workgroup adds 1 behind its last store
  double *state;                               // [C][SL_ROWS][64] device memory: where a chain's state rests during an evaluation
  double *trace;                               // [C][rpc][B7_SLICE_TRACE_WIDTH] device memory, zeroed by the caller; null: no trace
  int *trace_n;                                // [C] records written
  int rpc;
};

// ---- the slice sampler's hyper chain on the device (b7_gp_slice_sample): samplers/slice.lua:51-168 in its default mode (random
// direction, log space, step-out, per-dimension widths, max_step), one workgroup per chain, U updates per launch.
// Wave 0 IS the sampler: lane k holds component k of x0, direction, left, right, the widths and the bounds (D = d + 3 <= 35
// components); decisions that need all components go through ballots.  It runs the reference's statements until one of them
// asks for a density value that is neither known (the point an update starts from is the point the last one ended on) nor
// -inf (outside the bounds: no evaluation), leaves exp(theta) in red[8..] and a command word in red[48], and the whole
// workgroup runs gs_body<0> -- the instructions and operands of gp_small_kernel<0> -- on it.  The value is
// -(0.5 t0 + t1 + c0), b7_gp_nll_batch's host expression in its order.  All sampler arithmetic has contraction off.
// Draws: counter_rng.h, stream key(seed, chain); update g owns the counters 4096 g .. 4096 g + 4095 (layout there).
// Every loop is bounded: a step-out by max_step, the density requests of an update by max_evals (B7_SLICE_CAP), the inner
// loop below by U (max_evals + 2) rounds.
enum { SL_NEW = -1, SL_START = 0, SL_RIGHT = 1, SL_LEFT = 2, SL_SHRINK = 3 };  // 0..3: the trace's request kinds
constexpr int SL_ROWS = 10;  // rows of 64 doubles in a chain's state block
template <bool TWO, int KERN>
__global__ void __launch_bounds__(GS_THREADS) slice_chain_kernel(GsArgs a, SliceArgs s) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) double sm[];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double *red = sm + GS_RED_AT;
  double *hyp = red + 8;                              // [D] the hyper pack of the evaluation under way: exp(theta), the mean as it is
  int *ctl = reinterpret_cast<int *>(red + 48);       // 1: evaluate hyp, 0: the chain is done
  const int D = s.D, d = D - 3, U = s.U;
  const bool mine = lane < D;
  const uint64_t key = counter_key(s.seed, (uint64_t)c);
  const double nan = __builtin_nan(""), ninf = -__builtin_inf();
  // ---- the chain's state.  Per component (lane k of wave 0): x0, direction, left, right, dx, theta of the request under way,
  // the widths and the bounds; per chain: f(x0), the slice level Y, log u_Y, the shrink uniform.  There is no LDS left for it
  // (GS_LDS_DOUBLES) and the likelihood body leaves no registers: between two sampler sections it rests in the chain's block
  // of device memory (s.state: SL_ROWS rows of 64 doubles; the same lanes write and read it, nobody else does).  What steers
  // the control flow -- phase, counters, the value, the pivot word -- is wave-uniform and lives in scalar registers.
  double *st = s.state + (size_t)c * SL_ROWS * 64;
  double x0 = 0.0, dir = 0.0, left = 0.0, right = 0.0, dx = 0.0, th = 0.0, wd = 1.0, lo = 0.0, hi = 0.0;
  double fx0 = nan, Y = 0.0, val = 0.0, us = 0.0, luY = 0.0;
  auto save = [&]() {
    if (mine) st[lane] = x0, st[64 + lane] = dir, st[128 + lane] = left, st[192 + lane] = right, st[256 + lane] = dx, st[320 + lane] = th;
    if (lane == 0) st[576] = fx0, st[577] = Y, st[578] = luY, st[579] = us;
  };
  auto load = [&]() {
    if (mine) {
      x0 = st[lane], dir = st[64 + lane], left = st[128 + lane], right = st[192 + lane], dx = st[256 + lane], th = st[320 + lane];
      wd = st[384 + lane], lo = st[448 + lane], hi = st[512 + lane];
    }
    fx0 = st[576], Y = st[577], luY = st[578], us = st[579];
  };
  if (wave == 0) {
    if (mine) {
      x0 = s.theta0[(size_t)c * D + lane];
      st[384 + lane] = s.widths[lane], st[448 + lane] = s.lo[lane], st[512 + lane] = s.hi[lane];
    }
    save();
  }
  bool have_fx0 = false, have_val = false, dead = false;
  int phase = SL_NEW, itr = 0, nreq = 0, status = 0, u = 0, nev = 0, nrec = 0, shrink_i = 0, piv = 0;
  uint64_t base = 0;
  unsigned long long tick0 = 0;
  double *trace = s.trace ? s.trace + (size_t)c * s.rpc * B7_SLICE_TRACE_WIDTH : nullptr;
  // thread 0's value for the whole of wave 0, as a value the compiler knows to be uniform
  auto first_lane = [](double v) {
    const int l = __builtin_amdgcn_readfirstlane(__double2loint(v)), h = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(h, l);
  };

  // one trace record (wave 0, all lanes): eight header doubles, then two arrays of up to 64
  auto record = [&](double h0, double h1, double h2, double h3, double h4, double h5, double h6, double h7, double va, double vb) {
    if (!trace || nrec >= s.rpc) return;
    double *rec = trace + (size_t)nrec * B7_SLICE_TRACE_WIDTH;
    if (lane == 0) rec[0] = h0, rec[1] = h1, rec[2] = h2, rec[3] = h3, rec[4] = h4, rec[5] = h5, rec[6] = h6, rec[7] = h7;
    if (mine) rec[8 + lane] = va, rec[72 + lane] = vb;
    ++nrec;
  };
  // an update ends on (theta, value): out it goes, and the next one starts there
  auto finish = [&](double theta_k, double value, int st_bits) {
    const size_t at = (size_t)c * U + u;
    if (mine) s.theta_out[at * D + lane] = theta_k;
    if (lane == 0) s.value_out[at] = value, s.status_out[at] = st_bits;
    x0 = theta_k, fx0 = value, have_fx0 = true;
    ++u, phase = SL_NEW;
  };

  for (;;) {
    if (wave == 0) {
      int cmd = 0;
      load();
      if (have_val) {  // the evaluation that has just run: its record (theta and the pack are still where the request left them)
        record(1.0, (double)phase, us, 1.0, 0.0, val, first_lane((double)tick0), 0.0, th, mine ? hyp[lane] : 0.0);
      }
      for (;;) {
        if (phase == SL_NEW) {
          if (u >= U) break;  // cmd = 0
          if (dead) {         // status 16: not run (a failed pivot stopped the chain)
            finish(x0, fx0, 16);
            continue;
          }
          base = 4096ull * (s.update0 + (uint64_t)u);
          // direction = z / norm(z): the sum of squares ascending from 0.0, every product and every addition rounded (:80-82)
          const double z = mine ? counter_normal(key, base + lane) : 0.0;
          double ss = 0.0;
          for (int k = 0; k < D; ++k) {
            const double zk = __shfl(z, k);
            const double sq = zk * zk;
            ss = ss + sq;
          }
          dir = z / sqrt(ss);
          const double uY = counter_uniform(key, base + 64);
          luY = log(uY);
          const double ur = mine ? counter_uniform(key, base + 128 + lane) : 0.0;
          right = ur * wd;     // :114-115
          left = right - wd;
          record(0.0, (double)(s.update0 + (uint64_t)u), uY, luY, 0.0, 0.0, 0.0, 0.0, z, ur);
          nreq = 0, status = 0, itr = 0, shrink_i = 0, have_val = false;
          phase = SL_START;
        }
        if (have_val) {  // the answer to the request of `phase`
          have_val = false;
          if (piv != 0) {  // the plain factorisation failed: the chain stops on its last good point (status 8)
            finish(x0, phase == SL_START ? nan : fx0, status | 8);
            dead = true;
            continue;
          }
          if (phase == SL_START) {  // :106-111
            fx0 = val;
            Y = fx0 + luY;
            phase = SL_RIGHT, itr = 0;
          } else if (phase == SL_RIGHT) {  // :118-123
            if (val > Y && itr < s.max_step) {
              ++itr;
              right = right + wd;
            } else {
              phase = SL_LEFT, itr = 0;
            }
          } else if (phase == SL_LEFT) {  // :124-129
            if (val > Y && itr < s.max_step) {
              ++itr;
              left = left - wd;
            } else {
              phase = SL_SHRINK;
            }
          } else {  // :134-164
            bool accept = false;
            if (val != val) {
              status |= 1, accept = true;
            } else if (val > Y) {
              accept = true;
            } else if (__ballot(mine && dx == 0.0) != 0ull) {
              status |= 2, accept = true;
            }
            if (accept) {
              finish(th, val, status);  // x0 + direction * dx, :167: the request's own theta
              continue;
            }
            right = dx > 0.0 ? dx : right;  // :153-156
            left = dx < 0.0 ? dx : left;    // :158-161
            ++shrink_i;
          }
        }
        // ---- the request of the phase we are in
        if (nreq >= s.max_evals) {  // the cap: the update returns x0 unchanged (status 4)
          finish(x0, fx0, status | 4);
          continue;
        }
        ++nreq;
        bool reused = false;
        us = 0.0;
        if (phase == SL_START) {
          th = x0;
          reused = have_fx0;
        } else {
          if (phase == SL_SHRINK) {
            us = counter_uniform(key, base + 256 + (uint64_t)shrink_i);
            const double span = right - left;
            const double step = span * us;
            dx = left + step;
          } else {
            dx = phase == SL_RIGHT ? right : left;
          }
          const double mv = dir * dx;
          th = x0 + mv;
        }
        const bool inb = __ballot(mine && !(th >= lo && th <= hi)) == 0ull;  // a NaN fails both comparisons
        piv = 0;
        if (reused || !inb) {
          val = reused ? fx0 : ninf;
          record(1.0, (double)phase, us, inb ? 1.0 : 0.0, reused ? 1.0 : 0.0, val, 0.0, 0.0, th, 0.0);
          have_val = true;
          continue;
        }
        const double h = lane < d + 2 ? exp(th) : th;
        if (mine) hyp[lane] = h;
        cmd = 1;
        break;
      }
      save();
      if (lane == 0) ctl[0] = cmd;
    }
    __syncthreads();
    if (ctl[0] == 0) break;
    if (trace && tid == 0) tick0 = wall_clock64();
    double t0 = 0.0, t1 = 0.0;
    int *inf;
    gs_body<0, TWO, KERN, true>(a, 0, hyp, hyp[d], hyp[d + 1], hyp[d + 2], t0, t1, inf);
    if (wave == 0) {
      // -(0.5 t0 + t1 + c0): the host's expression (b7_gp_nll_batch), thread 0's terms for the whole wave
      const double half = 0.5 * t0;
      const double sum = half + t1;
      const double nll = sum + s.c0;
      val = first_lane(-nll);
      piv = __builtin_amdgcn_readfirstlane(inf[0]);
      if (trace && tid == 0) tick0 = wall_clock64() - tick0;
      ++nev;
      have_val = true;
    }
  }
  if (wave == 0 && lane == 0) {
    s.nevals_out[c] = nev;
    if (s.trace_n) s.trace_n[c] = nrec;
  }
  // the host makes ONE wait, on the counter: wave 0's stores are pushed out to system scope, then thread 0's release add
  __threadfence_system();
  __syncthreads();
  if (tid == 0) __hip_atomic_fetch_add(s.done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}


template <bool TWO, int KERN>
int slice_launch2(b7_ctx *c, const GsArgs &a, const SliceArgs &s, int C) {
  const size_t lds = sizeof(double) * GS_LDS_DOUBLES;
  static bool attr_done[64] = {false};
  if (c->device >= 64 || !attr_done[c->device]) {
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(slice_chain_kernel<TWO, KERN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (c->device < 64) attr_done[c->device] = true;
  }
  hipLaunchKernelGGL((slice_chain_kernel<TWO, KERN>), dim3(C), dim3(GS_THREADS), lds, c->stream, a, s);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}
template <int KERN>
int slice_launch_k(b7_ctx *c, const GsArgs &a, const SliceArgs &s, int C) {
  return a.N > NB ? slice_launch2<true, KERN>(c, a, s, C) : slice_launch2<false, KERN>(c, a, s, C);
}


// C chains of s.U slice-sampling updates of the resident data, one workgroup each (the caller has checked gp_small_applies)
int launch_slice_chain(b7_ctx *c, int C, const SliceArgs &s) {
  PhaseScope ps(c, "slice");
  GsArgs a = {};
  a.xobs = (const double *)c->xobs.p;
  a.y = (const double *)c->ybuf.p;
  a.N = c->N, a.d = c->dfit, a.dpad = c->dpad, a.B = 1;
  return c->kernel == B7_KERNEL_MATERN52 ? slice_launch_k<B7_KERNEL_MATERN52>(c, a, s, C) : slice_launch_k<B7_KERNEL_ARDSE>(c, a, s, C);
}

}  // namespace

int b7_gp_slice_sample(b7_ctx *c, int C, int U, const double *theta0, const double *lo, const double *hi, const double *widths,
                       int max_step, int max_evals, uint64_t seed, uint64_t update0, double *theta_out, double *value_out,
                       int *status_out, int *nevals_out) {
  if (!c) return B7_ERR_INVALID;
  if (!theta0 || !lo || !hi || !widths || !theta_out || !value_out || !status_out || !nevals_out)
    return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: NULL argument");
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "gp_slice_sample: no resident data (call b7_gp_set_data first)");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_slice_sample: %d response columns (one response column only)", c->ycols);
  if (c->N > 128) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_slice_sample: N = %d observations (N <= 128 only)", c->N);
  if (c->dfit > 32) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_slice_sample: d = %d input dimensions (d <= 32 only)", c->dfit);
  if (!gp_small_applies(c)) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_slice_sample: small sets padded to 128 keep the general path (not built here)");
  const int D = c->dfit + 3;
  if (C < 1 || C > B7_SLICE_MAX_CHAINS) return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: C = %d chains (1..%d)", C, B7_SLICE_MAX_CHAINS);
  if (U < 1) return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: U = %d updates (>= 1)", U);
  if (max_step < 0) return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: max_step = %d (>= 0)", max_step);
  if (max_evals < 1 || max_evals > B7_SLICE_MAX_EVALS)
    return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: max_evals = %d (1..%d)", max_evals, B7_SLICE_MAX_EVALS);
  if ((int64_t)U * max_evals > B7_SLICE_MAX_WORK)
    return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: U * max_evals = %lld evaluations per chain (<= %d)", (long long)U * max_evals, B7_SLICE_MAX_WORK);
  if (D > 64) return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: d + 3 = %d components (<= 64)", D);
  for (int k = 0; k < D; ++k) {
    if (!(widths[k] > 0.0)) return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: widths[%d] must be > 0", k);
    if (!(lo[k] <= hi[k])) return b7_fail(c, B7_ERR_INVALID, "gp_slice_sample: lo[%d] > hi[%d]", k, k);
  }
  B7_HIP(c, hipSetDevice(c->device));
  // ONE block of pinned, device-mapped host memory, in and out:
  // [C x D theta0 | D lo | D hi | D widths][C x U x D theta][C x U value][C x U status][C evaluation counts][completion counter]
  const size_t CU = (size_t)C * U, in_doubles = (size_t)C * D + 3 * (size_t)D, out_doubles = CU * D + CU;
  const size_t need = sizeof(double) * (in_doubles + out_doubles) + sizeof(int) * (CU + C + 4);
  B7_TRY(b7_pin_ensure(c, c->pin_slice, need, true));
  double *in = static_cast<double *>(c->pin_slice.host), *th_h = in + in_doubles, *val_h = th_h + CU * D;
  int *st_h = reinterpret_cast<int *>(val_h + CU), *nev_h = st_h + CU;
  volatile unsigned *done = reinterpret_cast<volatile unsigned *>(nev_h + C);
  memcpy(in, theta0, sizeof(double) * (size_t)C * D);
  memcpy(in + (size_t)C * D, lo, sizeof(double) * D);
  memcpy(in + (size_t)C * D + D, hi, sizeof(double) * D);
  memcpy(in + (size_t)C * D + 2 * (size_t)D, widths, sizeof(double) * D);
  *done = 0u;
  double *in_d = static_cast<double *>(c->pin_slice.dev), *th_d = in_d + in_doubles, *val_d = th_d + CU * D;
  int *st_d = reinterpret_cast<int *>(val_d + CU), *nev_d = st_d + CU;
  SliceArgs s = {};
  s.D = D, s.U = U, s.max_step = max_step, s.max_evals = max_evals;
  s.seed = seed, s.update0 = update0;
  s.c0 = 0.5 * c->N * log(2.0 * M_PI);  // b7_gp_nll_batch's constant
  s.theta0 = in_d, s.lo = in_d + (size_t)C * D, s.hi = s.lo + D, s.widths = s.hi + D;
  s.theta_out = th_d, s.value_out = val_d, s.status_out = st_d, s.nevals_out = nev_d;
  s.done = reinterpret_cast<unsigned *>(nev_d + C);
  B7_TRY(b7_ensure(c, c->slice_state, sizeof(double) * (size_t)C * SL_ROWS * 64));
  s.state = static_cast<double *>(c->slice_state.p);
  c->slice_trace_C = 0;
  if (c->slice_trace_rpc > 0) {
    const size_t rec_bytes = sizeof(double) * (size_t)C * c->slice_trace_rpc * B7_SLICE_TRACE_WIDTH;
    B7_TRY(b7_ensure(c, c->slice_trace, rec_bytes + sizeof(int) * (size_t)C));
    B7_HIP(c, hipMemsetAsync(c->slice_trace.p, 0, rec_bytes + sizeof(int) * (size_t)C, c->stream));
    s.trace = static_cast<double *>(c->slice_trace.p);
    s.trace_n = reinterpret_cast<int *>(static_cast<char *>(c->slice_trace.p) + rec_bytes);
    s.rpc = c->slice_trace_rpc;
  }
  B7_TRY(launch_slice_chain(c, C, s));
  // one wait: the counter every workgroup raises behind its last store; a launch that has not answered after B7_SPIN_US is
  // waited for the ordinary way (which also surfaces a fault)
  bool answered = false;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0; !answered && c->spin_us > 0; ++spins) {
    answered = __atomic_load_n(const_cast<const unsigned *>(done), __ATOMIC_ACQUIRE) == (unsigned)C;
    if (!answered && (spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->spin_us)) break;
  }
  if (!answered || c->slice_trace_rpc > 0) B7_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(theta_out, th_h, sizeof(double) * CU * D);
  memcpy(value_out, val_h, sizeof(double) * CU);
  memcpy(status_out, st_h, sizeof(int) * CU);
  memcpy(nevals_out, nev_h, sizeof(int) * C);
  if (c->slice_trace_rpc > 0) c->slice_trace_C = C, c->slice_trace_D = D;
  return B7_OK;
}

int b7_gp_slice_trace_enable(b7_ctx *c, int records_per_chain) {
  if (!c) return B7_ERR_INVALID;
  if (records_per_chain < 0 || records_per_chain > B7_SLICE_MAX_WORK + B7_SLICE_MAX_WORK / 2)
    return b7_fail(c, B7_ERR_INVALID, "gp_slice_trace_enable: records_per_chain = %d (0..%d)", records_per_chain,
                   B7_SLICE_MAX_WORK + B7_SLICE_MAX_WORK / 2);
  c->slice_trace_rpc = records_per_chain;
  c->slice_trace_C = 0;
  return B7_OK;
}

int b7_gp_slice_trace(b7_ctx *c, int chain, double *records, int *n_records) {
  if (!c) return B7_ERR_INVALID;
  if (!n_records) return b7_fail(c, B7_ERR_INVALID, "gp_slice_trace: NULL argument");
  if (c->slice_trace_C < 1 || c->slice_trace_rpc < 1)
    return b7_fail(c, B7_ERR_STATE, "gp_slice_trace: no traced b7_gp_slice_sample (b7_gp_slice_trace_enable first)");
  if (chain < 0 || chain >= c->slice_trace_C) return b7_fail(c, B7_ERR_INVALID, "gp_slice_trace: chain %d of %d", chain, c->slice_trace_C);
  B7_HIP(c, hipSetDevice(c->device));
  const size_t per_chain = (size_t)c->slice_trace_rpc * B7_SLICE_TRACE_WIDTH;
  const char *base = static_cast<const char *>(c->slice_trace.p);
  int n = 0;
  B7_HIP(c, hipMemcpy(&n, base + sizeof(double) * per_chain * c->slice_trace_C + sizeof(int) * (size_t)chain, sizeof(int), hipMemcpyDeviceToHost));
  if (n < 0 || n > c->slice_trace_rpc) return b7_fail(c, B7_ERR_HIP, "gp_slice_trace: record count %d out of range", n);
  if (records && n > 0)
    B7_HIP(c, hipMemcpy(records, base + sizeof(double) * per_chain * chain, sizeof(double) * (size_t)n * B7_SLICE_TRACE_WIDTH, hipMemcpyDeviceToHost));
  *n_records = n;
  return B7_OK;
}

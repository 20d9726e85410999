// The slab walk: 64 query rows held as MFMA fragments while the pre-scaled observations stream past them, slab by slab.
//
// ksx_kernel (covar.hip) and believer_kernel (batch.hip) are this walk with different riders and tile bodies, so a downdated
// variance is made of the covariance entries the posterior itself was made of, and the sum over the observations has one order
// whatever the grid's size.  kg_kernel (kg.hip) keeps a copy of its own (its header says why); tests/test_gpu_cov_walk_bits.py
// pins the bits of all three.
//
// A block of 256 threads owns 64 query rows (16 per wave) and walks the observations in slabs of 64 rows (32 for dpad >= 48),
// double-buffered in LDS: the next slab is prefetched into registers while the current one is consumed, one barrier per slab.
// The query tile is dead once its fragments sit in registers, before the first slab is consumed, so the two slab buffers live
// in the SAME LDS region (50 -> 34 KB per workgroup at DPAD 32, 67 -> 34 at 64, 99 -> 50 at 96: three workgroups per CU, the
// register file's limit); that costs two barriers in the prologue.  The row stride DPAD + 1 is odd: conflict-free for the
// fused ds_read2_b64 fragment reads (gemm_f64.h).
//
// A kernel brings four inlined callables:
//   stage()                       writes its own LDS (from extra() on) before the first barrier
//   rider_load(slab), rider_store(buf)
//                                 what travels with a slab beside the rows and zs/2 -- alpha, w_j: one word per observation
//                                 row -- global memory to the kernel's registers, then registers to rider() in LDS; run by the
//                                 threads (tid < KO) that move the row's zs/2, under their guard
//   tile(slab, buf, t, bf)        the 16 observations t of the slab in buffer buf: bf[k4] is this lane's fragment (observation
//                                 16 t + lr, k = 4 k4 + lq); their zs/2 is zs()[buf KO + 16 t + lr].  The body issues the MFMAs
//                                 itself (dist / cov below, or ksx_kernel's ablation arms).
// begin() is the prologue, run() the loop; a kernel reads xs() in between.  A column pass has nslab = 0; K(X,X)'s blockIdx.y
// split has slab0 != 0.
#pragma once
#include "b7_internal.h"
#include "gemm_f64.h"
#include "ksx_exp.h"

constexpr int KSX_Q = 64;  // query rows per block (16 per wave)

// The tile of one dpad class.  RW: the rider's LDS words per observation row.
template <int DPAD, int RW>
struct KsxTile {
  static constexpr int Q = KSX_Q;
  // observation slab: 64 rows, 32 for the wide classes so that two blocks still fit a CU's LDS
  // (measured at DPAD = 64 with 64-row slabs: 1 block/CU, 2.07 TB/s against 3.97 TB/s at DPAD = 32)
  static constexpr int KO = DPAD >= 48 ? 32 : 64;
  static constexpr int TPR = 256 / KO;                 // staging threads per slab row
  static constexpr int HALF = DPAD >> 1;               // 16-byte chunks per row
  static constexpr int NCH = (HALF + TPR - 1) / TPR;   // chunks per staging thread
  static constexpr int KSTEPS = DPAD / 4;
  static constexpr int STRIDE = DPAD + 1;
  static constexpr int R0 = (Q > 2 * KO ? Q : 2 * KO) * STRIDE;  // the query tile, then the two slab buffers
  // LDS, in doubles: R0 | 2 KO zs/2 of the slab | 2 KO RW rider | Q xs/2 of the queries | 128 amp * 2^(j/128) | the kernel's own
  static constexpr int RIDER = R0 + 2 * KO, XS = RIDER + 2 * KO * RW, TAB = XS + Q, EXTRA = TAB + 128;
  static constexpr size_t lds_bytes(int extra_doubles) { return sizeof(double) * (size_t)(EXTRA + extra_doubles); }
};

template <int DPAD, int RW>
struct KsxWalk {
  using T = KsxTile<DPAD, RW>;
  double *const sm;
  const double *const zsc, *const zsh;    // the pre-scaled observations (rows of DPAD) and their zs/2
  const int tid, lane, wave, lr, lq;
  double qf[T::KSTEPS];                   // this lane's query fragments: query row (wave*16 + lr), k = 4 k4 + lq
  d2_t pre[T::NCH];                       // the prefetched slab
  double pre_h = 0.0;

  __device__ __forceinline__ KsxWalk(double *sm_, const double *zsc_, const double *zsh_)
      : sm(sm_), zsc(zsc_), zsh(zsh_), tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), lr(lane & 15), lq(lane >> 4) {}
  __device__ __forceinline__ double *zs() const { return sm + T::R0; }      // 2 x KO: zs/2 of the slab in each buffer
  __device__ __forceinline__ double *rider() const { return sm + T::RIDER; }
  __device__ __forceinline__ double *xs() const { return sm + T::XS; }      // xs/2 of the block's queries, after begin()
  __device__ __forceinline__ double *tab() const { return sm + T::TAB; }
  __device__ __forceinline__ double *extra() const { return sm + T::EXTRA; }

  template <class RiderLoad>
  __device__ __forceinline__ void load_slab(int s, RiderLoad &rider_load) {
    const int srow = tid / T::TPR, sq4 = tid % T::TPR;
    const double *src = zsc + (int64_t)(s * T::KO + srow) * DPAD;
#pragma unroll
    for (int i = 0; i < T::NCH; ++i) {
      const int kc = i * T::TPR + sq4;
      if (kc < T::HALF) pre[i] = *reinterpret_cast<const d2_t *>(src + 2 * kc);
    }
    if (tid < T::KO) {
      pre_h = zsh[s * T::KO + tid];
      rider_load(s);
    }
  }
  template <class RiderStore>
  __device__ __forceinline__ void store_slab(int buf, RiderStore &rider_store) {
    const int srow = tid / T::TPR, sq4 = tid % T::TPR;
    double *dst = sm + buf * T::KO * T::STRIDE + srow * T::STRIDE;
#pragma unroll
    for (int i = 0; i < T::NCH; ++i) {
      const int kc = i * T::TPR + sq4;
      if (kc < T::HALF) {
        dst[2 * kc] = pre[i][0];
        dst[2 * kc + 1] = pre[i][1];
      }
    }
    if (tid < T::KO) {
      zs()[buf * T::KO + tid] = pre_h;
      rider_store(buf);
    }
  }

  // xq: query rows, row-major with d columns; the block's rows start at qbase, rows beyond Mtotal - 1 are clamped (they produce
  // values nobody reads).  w: the weights 1/ls (DPAD of them).
  template <class Stage, class RiderLoad, class RiderStore>
  __device__ __forceinline__ void begin(const double *xq, int64_t qbase, int64_t Mtotal, int d, const double *w, double amp,
                                        int slab0, int nslab, Stage &&stage, RiderLoad &rider_load, RiderStore &rider_store) {
    double *sq = sm;  // Q x STRIDE, prologue only
    if (tid < 128) tab()[tid] = amp * b7_exp2_tab_dev[tid];
    {  // query tile (zero-padded columns): 64 rows, 4 threads per row
      const int qrow = tid >> 2, qq4 = tid & 3;
      int64_t g = qbase + qrow;
      if (g > Mtotal - 1) g = Mtotal - 1;
      for (int k = qq4; k < DPAD; k += 4) sq[qrow * T::STRIDE + k] = (k < d) ? xq[g * d + k] : 0.0;
    }
    stage();
    if (nslab > 0) load_slab(slab0, rider_load);
    __syncthreads();  // query tile visible
    if (tid < T::Q) {
      double s = 0.0;
      for (int k = 0; k < DPAD; ++k) {
        double x = sq[tid * T::STRIDE + k];
        s += (x * x) * w[k];  // X_ss = (X.^2) * inv_ls, utils/math.lua:78
      }
      xs()[tid] = 0.5 * s;
    }
#pragma unroll
    for (int k4 = 0; k4 < T::KSTEPS; ++k4) qf[k4] = sq[(wave * 16 + lr) * T::STRIDE + lq + 4 * k4];
    __syncthreads();  // every wave holds its fragments, xs is complete: the region now belongs to the slabs
    if (nslab > 0) store_slab(0, rider_store);
    __syncthreads();
  }

  template <class RiderLoad, class RiderStore, class Tile>
  __device__ __forceinline__ void run(int slab0, int nslab, RiderLoad &rider_load, RiderStore &rider_store, Tile &&tile) {
    int cur = 0;
    for (int s = 0; s < nslab; ++s) {
      const bool more = (s + 1) < nslab;
      if (more) load_slab(slab0 + s + 1, rider_load);
      const double *sob = sm + cur * T::KO * T::STRIDE;
#pragma unroll
      for (int t = 0; t < T::KO / 16; ++t) {
        const double *ob = sob + (t * 16 + lr) * T::STRIDE + lq;
        double bf[T::KSTEPS];
#pragma unroll
        for (int k4 = 0; k4 < T::KSTEPS; ++k4) bf[k4] = ob[4 * k4];
        tile(slab0 + s, cur, t, bf);
      }
      if (more) store_slab(cur ^ 1, rider_store);
      __syncthreads();
      cur ^= 1;
    }
  }

  // One 16 x 16 tile with the queries as the A operand, in two steps (a kernel reads the columns' scalars in between, behind the
  // MFMAs): dist = D[query lq + 4 r][column lr] of the columns whose fragments are bf; cov = their covariances, hq[r] being
  // xs/2 of query lq + 4 r and hk zs/2 of column lr.
  __device__ __forceinline__ d4_t dist(const double (&bf)[T::KSTEPS]) const {
    d4_t c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k4 = 0; k4 < T::KSTEPS; ++k4) c = mfma_f64(qf[k4], bf[k4], c);
    return c;
  }
  __device__ __forceinline__ void arg4(const d4_t &c, const double (&hq)[4], double hk, double (&arg)[4]) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) arg[r] = (c[r] - hq[r]) - hk;  // = -1/2 * (((-2 c) + xs) + zs), utils/math.lua:82
  }
  template <int KERN>
  __device__ __forceinline__ void cov(const d4_t &c, const double (&hq)[4], double hk, double (&kv)[4]) const {
    double arg[4];
    arg4(c, hq, hk, arg);
    cov_nonpos4<KERN>(arg, tab(), kv);  // :106 clamp(0, huge) on the distance (NaN passes), amp * exp(-D/2) (ARD-SE)
  }
};

// ksx_for_class: (c->dpad, c->kernel) -> f(KsxClass<DPAD, KERN>{}): the built classes of the walk's kernels.  who: the kernel family, for the message
template <int DPAD_, int KERN_>
struct KsxClass {
  static constexpr int DPAD = DPAD_, KERN = KERN_;
};
template <int KERN, class F>
int ksx_dispatch_dpad(b7_ctx *c, const char *who, F &&f) {
  switch (c->dpad) {
    case 4: return f(KsxClass<4, KERN>{});
    case 8: return f(KsxClass<8, KERN>{});
    case 16: return f(KsxClass<16, KERN>{});
    case 32: return f(KsxClass<32, KERN>{});
    case 48: return f(KsxClass<48, KERN>{});
    case 64: return f(KsxClass<64, KERN>{});
    case 96: return f(KsxClass<96, KERN>{});
    default: return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: dpad %d is not a built class", who, c->dpad);
  }
}
template <class F>
int ksx_for_class(b7_ctx *c, const char *who, F &&f) {
  if (c->kernel == B7_KERNEL_MATERN52) return ksx_dispatch_dpad<B7_KERNEL_MATERN52>(c, who, f);
  return ksx_dispatch_dpad<B7_KERNEL_ARDSE>(c, who, f);
}

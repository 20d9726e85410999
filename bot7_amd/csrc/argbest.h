// The arg-best reduction of every pick kernel, once: the (value, row) record, the five orderings, the workgroup reduction, the kernel
// of a pass over M rows that leaves one partial per workgroup, and the kernel that folds the partials into taken[j].
//
// An ordering is a functor bool(const ArgBest &a, const ArgBest &b): a is STRICTLY preferred to b.  A record with i < 0 is "none": it
// is preferred to nothing and everything is preferred to it.  The result of a reduction must not depend on its shape (lanes, waves,
// workgroups, the grid-stride order), which holds exactly when the ordering is a strict total order over the candidates that can
// reach it; each functor below states what a NaN does.  skips_nan: the ordering is total only without NaNs, so whoever feeds it keeps
// them out ahead of the comparison (the part kernel below does; hvi_body and ts_starts_kernel, which keep loops of their own, do too).
//
// ts_feas.hip's (class, key, row) record and its four-paths-at-a-time fold are a different shape and stay there.
#pragma once
#include <hip/hip_runtime.h>

struct ArgBest {
  double v;
  long long i;  // the row, 0-based; < 0: none
};

constexpr int ARGBEST_MAX_EXCL = 16;  // rows a pass can leave out: B7_BATCH_MAX, B7_REFINE_MAX_STARTS and B7_KG_MAX_POINTS are all 16

// TH's max (score.hip, refine.hip): the larger value, ties to the lower row; the FIRST NaN wins over everything.  Total.
struct OrderMaxNanFirst {
  static constexpr bool skips_nan = false;
  __device__ __forceinline__ bool operator()(const ArgBest &a, const ArgBest &b) const {
    if (b.i < 0) return a.i >= 0;
    if (a.i < 0) return false;
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an || bn) return an && (!bn || a.i < b.i);
    return (a.v > b.v) || (a.v == b.v && a.i < b.i);
  }
};
// A sample path's first minimum (rff.hip): the smaller value, ties to the lower row; a NaN loses to every number (NaNs among
// themselves: the lower row), so it is picked only where nothing else is left.  Total.
struct OrderMinNanLast {
  static constexpr bool skips_nan = false;
  __device__ __forceinline__ bool operator()(const ArgBest &a, const ArgBest &b) const {
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an != bn) return bn;
    if (!an && a.v != b.v) return a.v < b.v;
    return a.i < b.i;
  }
};
// The hypervolume improvement's maximum (ts_hvi.hip): the larger value, ties to the lower row.  NOT total if a NaN gets in (it
// compares unequal to everything and then "larger" to nothing): the caller skips NaN scores before the comparison, as hvi_body does.
struct OrderMaxNoNan {
  static constexpr bool skips_nan = true;
  __device__ __forceinline__ bool operator()(const ArgBest &a, const ArgBest &b) const {
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    if (a.v != b.v) return a.v > b.v;
    return a.i < b.i;
  }
};
// The lowest marginal mean (kg.hip): the smaller value, ties to the lower row; a NaN counts as +inf, so n <= M rows are always
// found.  Total.
struct OrderMinNanInf {
  static constexpr bool skips_nan = false;
  __device__ __forceinline__ bool operator()(const ArgBest &a, const ArgBest &b) const {
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    const double x = (a.v != a.v) ? INFINITY : a.v, y = (b.v != b.v) ? INFINITY : b.v;
    return x < y || (x == y && a.i < b.i);
  }
};
// Plain ascending (value, row) (ts_refine.hip's starts, which also use it as "strictly after the previous pick").  NOT total with a
// NaN (it is before and after nothing): the caller skips NaN values, as ts_starts_kernel does.
struct OrderMin {
  static constexpr bool skips_nan = true;
  __device__ __forceinline__ bool operator()(const ArgBest &a, const ArgBest &b) const {
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    return a.v < b.v || (a.v == b.v && a.i < b.i);
  }
};

template <class Order>
__device__ __forceinline__ ArgBest wave_best(ArgBest x) {
  for (int o = 32; o > 0; o >>= 1) {
    ArgBest y;
    y.v = __shfl_xor(x.v, o);
    y.i = __shfl_xor(x.i, o);
    if (Order()(y, x)) x = y;
  }
  return x;
}
// The best of a workgroup of up to 256 threads to every thread of it: wave shuffles, one LDS slot per wave (sh: 4 records), two
// barriers.  Every thread calls.  NOT safe to call twice in a row on the same sh: all threads read sh[0] after the last barrier and
// the next call's first wave writes sh[0] with no barrier between.  A kernel that calls it in a loop puts a __syncthreads() ahead of
// every call but the first; the single-call kernels on the nomination's path pay for none.
template <class Order>
__device__ __forceinline__ ArgBest block_best(ArgBest x, ArgBest *sh) {
  x = wave_best<Order>(x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = x;
  __syncthreads();
  if (wave == 0) {
    ArgBest y = (lane < (int)(blockDim.x >> 6)) ? sh[lane] : ArgBest{0.0, -1};
    y = wave_best<Order>(y);
    if (lane == 0) sh[0] = y;
  }
  __syncthreads();
  return sh[0];
}

// is row one of ex[0 .. ARGBEST_MAX_EXCL)?  (unused entries hold -1, which no row is)
__device__ __forceinline__ bool argbest_excluded(const long long (&ex)[ARGBEST_MAX_EXCL], long long row) {
  bool out = false;
#pragma unroll
  for (int e = 0; e < ARGBEST_MAX_EXCL; ++e) out = out || ex[e] == row;
  return out;
}
// the exclusion list excl[0 .. n) into registers.  excl has room for ARGBEST_MAX_EXCL entries whatever n is (every caller's list
// does): all of it is fetched at once and the entries from n on are replaced, with no chain of branches ahead of the kernel's loop
__device__ __forceinline__ void argbest_load_excl(const long long *__restrict__ excl, int n, long long (&ex)[ARGBEST_MAX_EXCL]) {
#pragma unroll
  for (int e = 0; e < ARGBEST_MAX_EXCL; ++e) ex[e] = -1;
  if (n <= 0) return;  // (excl may be null then)
#pragma unroll
  for (int e = 0; e < ARGBEST_MAX_EXCL; ++e) {
    const long long row = excl[e];
    ex[e] = (e < n) ? row : -1;
  }
}

// the plainest row loader: p[row * stride] (a vector: stride 1; column j of an [M][q] buffer: p = buf + j, stride q)
struct ArgLoadStrided {
  const double *p;
  long long stride;
  __device__ __forceinline__ double operator()(long long row) const { return p[row * stride]; }
};

namespace {  // (kernels have internal linkage in every translation unit of the library)

// One pass: the workgroup's best of load(row) over the rows of its grid-stride slice that are none of excl[0 .. n), into
// part[blockIdx.x].  load: a functor double(long long row).
template <class Order, class Load>
__global__ void __launch_bounds__(256)
    argbest_part_kernel(Load load, long long M, const long long *__restrict__ excl, int n, ArgBest *__restrict__ part) {
  __shared__ ArgBest sh[4];
  long long ex[ARGBEST_MAX_EXCL];
  argbest_load_excl(excl, n, ex);
  ArgBest b{0.0, -1};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < M; r += stride) {
    if (argbest_excluded(ex, r)) continue;
    const ArgBest cnd{load(r), r};
    if (Order::skips_nan && cnd.v != cnd.v) continue;
    if (Order()(cnd, b)) b = cnd;
  }
  b = block_best<Order>(b, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}
// the n partials of a pass into taken[j] (-1: no row was left) and, where val is given, val[j] (0.0 with no row)
template <class Order>
__global__ void __launch_bounds__(256)
    argbest_final_kernel(const ArgBest *__restrict__ part, int n, int j, long long *__restrict__ taken, double *__restrict__ val) {
  __shared__ ArgBest sh[4];
  ArgBest b{0.0, -1};
  for (int e = threadIdx.x; e < n; e += blockDim.x)
    if (Order()(part[e], b)) b = part[e];
  b = block_best<Order>(b, sh);
  if (threadIdx.x == 0) {
    taken[j] = b.i;
    if (val) val[j] = b.v;
  }
}

}  // namespace

// workgroups of a pass over M rows: one per 256 rows, 1024 at the most (beyond 262 144 rows the grid-stride loop takes another trip)
static inline int argbest_blocks(long long M) {
  const long long b = (M + 255) / 256;
  return (int)(b < 1024 ? b : 1024);
}

// pick j of a chain: a pass of nblk workgroups over M rows, the rows taken[0 .. j) left out, then taken[j] (and val[j]) on the device
template <class Order, class Load>
static inline void launch_argbest(hipStream_t stream, Load load, long long M, int nblk, ArgBest *part, int j, long long *taken, double *val) {
  hipLaunchKernelGGL((argbest_part_kernel<Order, Load>), dim3(nblk), dim3(256), 0, stream, load, M, (const long long *)taken, j, part);
  hipLaunchKernelGGL(argbest_final_kernel<Order>, dim3(1), dim3(256), 0, stream, (const ArgBest *)part, nblk, j, taken, val);
}

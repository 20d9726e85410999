// The candidate grid's entry points: generation (Sobol, counter-based uniform, torch.rand's stream), the one-sided affine
// maps, upload / download and stable row deletion.  The kernels are in sobol.hip.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "b7_internal.h"

static double *cur_grid(b7_ctx *c) { return (double *)c->grid[c->grid_cur].p; }

static void invalidate_predictions(b7_ctx *c) {
  c->predicted = false;
  acc_forget(c);
  feas_forget(c);
  post_forget(c);
  c->Mfeat = 0;  // DNGO features belong to the grid they were computed from
  c->win_valid = false;  // so does the winner's row of the last exchange
}

static int group_guard(b7_ctx *c, const char *who) {
  if (c->group && !c->group_busy)
    return b7_fail(c, B7_ERR_STATE, "%s: this context's grid is a shard of a group; use the b7_group_grid_* calls", who);
  return B7_OK;
}

// Stable deletion of candidate row local_idx1 (utils/tensor.lua:158-170), enqueued on the context's stream.  With row_out
// the removed row is copied out first and the stream is synchronised.
int grid_drop_row(b7_ctx *c, int64_t idx1, double *row_out) {
  B7_TRY(group_guard(c, "grid_remove"));
  if (idx1 < 1 || idx1 > c->M)
    return b7_fail(c, B7_ERR_INVALID, "grid_remove: index %lld outside [1, %lld]", (long long)idx1, (long long)c->M);
  B7_HIP(c, hipSetDevice(c->device));
  if (row_out)
    B7_HIP(c, hipMemcpyAsync(row_out, cur_grid(c) + (idx1 - 1) * c->d, sizeof(double) * c->d, hipMemcpyDeviceToHost,
                             c->stream));
  const int other = c->grid_cur ^ 1;
  B7_TRY(b7_ensure(c, c->grid[other], sizeof(double) * (size_t)c->M * c->d));
  B7_TRY(launch_remove_row(c, cur_grid(c), (double *)c->grid[other].p, c->M, c->d, idx1 - 1));
  c->grid_cur = other;
  c->M -= 1;
  invalidate_predictions(c);
  if (row_out) B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

static int grid_alloc(b7_ctx *c, int64_t M, int d) {
  B7_TRY(group_guard(c, "grid"));
  if (M < 0 || d < 1) return b7_fail(c, B7_ERR_INVALID, "grid: size %lld dims %d", (long long)M, d);
  if (d > B7_MAX_D) return b7_fail(c, B7_ERR_UNSUPPORTED, "grid: dims %d > %d", d, B7_MAX_D);
  B7_HIP(c, hipSetDevice(c->device));
  c->grid_cur = 0;
  B7_TRY(b7_ensure(c, c->grid[0], sizeof(double) * (size_t)M * d));
  c->M = M;
  c->d = d;
  invalidate_predictions(c);
  return B7_OK;
}

static int grid_copy_out(b7_ctx *c, double *out_host) {
  if (out_host && c->M > 0)
    B7_HIP(c, hipMemcpyAsync(out_host, cur_grid(c), sizeof(double) * (size_t)c->M * c->d, hipMemcpyDeviceToHost,
                             c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

// grids/sobol.lua:82-85, grids/random.lua:29-32: only one of mins / maxes given.  The shift / scale uses the column minima /
// maxima of the WHOLE grid: with a communicator the shards' extremes are combined by one all-reduce (min / max of d doubles).
// That makes the call COLLECTIVE, so a rank that failed before it (rc_before: a bad argument, an allocation) still enters it:
// the reduced vector carries one more element, a status that the failing rank sets to the value that wins the reduction
// (-inf under MIN, +inf under MAX), and every rank returns an error together instead of the others waiting for ever.
static int onesided(b7_ctx *c, const double *mins, const double *maxes, int rc_before) {
  const bool collective = c->comm && c->comm_world > 1;
  if (rc_before != B7_OK && !collective) return rc_before;
  const int d = (rc_before == B7_OK) ? c->d : 0;
  std::vector<double> ext(2 * (size_t)B7_MAX_D + 2);
  double *lo = ext.data(), *hi = ext.data() + B7_MAX_D + 1;
  for (int k = 0; k <= B7_MAX_D; ++k) lo[k] = INFINITY, hi[k] = -INFINITY;  // an empty shard constrains nothing
  int rc = rc_before;
  const std::string own = c->err;
  if (rc == B7_OK && c->M > 0) {
    std::vector<double> cmin(d), cmax(d);
    rc = b7_grid_colrange(c, cmin.data(), cmax.data());
    if (rc == B7_OK) {
      memcpy(lo, cmin.data(), sizeof(double) * d);
      memcpy(hi, cmax.data(), sizeof(double) * d);
    }
  }
  const std::string own2 = rc != B7_OK ? c->err : own;
  double *use = mins ? lo : hi;
  if (collective) {
    // every rank reduces the same B7_MAX_D + 1 values whatever its own d (a failed rank may not know it): the extremes, then
    // the status
    use[B7_MAX_D] = rc == B7_OK ? (mins ? INFINITY : -INFINITY) : (mins ? -INFINITY : INFINITY);
    const int rcc = b7_comm_allreduce_f64(c, use, B7_MAX_D + 1, mins ? B7_COMM_MIN : B7_COMM_MAX);
    if (rc != B7_OK) {
      c->err = own2;
      return rc;
    }
    if (rcc != B7_OK) return rcc;
    if (use[B7_MAX_D] == (mins ? -INFINITY : INFINITY))
      return b7_fail(c, B7_ERR_COMM, "one-sided grid map: another rank failed before the exchange of the column extremes; no rank maps its shard");
  }
  if (rc != B7_OK) return rc;
  if (c->M == 0) return B7_OK;
  return b7_grid_apply_onesided(c, mins, maxes, use);
}

static int grid_sobol_local(b7_ctx *c, int64_t size, int dims, int64_t skip, const double *mins, const double *maxes) {
  if (size < 0 || skip < 0) return b7_fail(c, B7_ERR_INVALID, "sobol: size %lld skip %lld", (long long)size, (long long)skip);
  if (dims < 1 || dims >= 40)  // assert(C.dims and C.dims < C.max_dims), grids/sobol.lua:36
    return b7_fail(c, B7_ERR_RANGE, "sobol: dims %d not in [1, 39] (grids/sobol.lua:36)", dims);
  // "Too many calls": lo0(seed) must stay <= 30 (grids/sobol.lua:317-324) -> seed <= 2^30 - 2
  if (size > 0 && size + skip - 1 > ((int64_t)1 << 30) - 2)
    return b7_fail(c, B7_ERR_RANGE, "sobol: point index %lld beyond 2^30-2 (grids/sobol.lua:317-324)",
                   (long long)(size + skip - 1));
  const bool both = mins && maxes;
  B7_TRY(grid_alloc(c, size, dims));
  return launch_sobol(c, cur_grid(c), size, dims, skip, both ? mins : nullptr, both ? maxes : nullptr);
}

static int grid_random_local(b7_ctx *c, int64_t size, int dims, uint64_t seed, int64_t row_offset, const double *mins,
                             const double *maxes) {
  if (size < 0 || row_offset < 0) return b7_fail(c, B7_ERR_INVALID, "random grid: size/offset negative");
  const bool both = mins && maxes;
  B7_TRY(grid_alloc(c, size, dims));
  return launch_random_grid(c, cur_grid(c), size, dims, seed, row_offset, both ? mins : nullptr, both ? maxes : nullptr);
}

// ---- torch.rand's own stream (grids/random.lua:24) ---------------------------------------------------------------------
// Torch7's CPU generator is MT19937 (TH/THRandom.c) [public knowledge, not in the reference tree]: manualSeed(s) is
// init_genrand(s), THRandom_random the tempered 32-bit output, and torch.rand fills a tensor in row-major order.  Two
// generations of TH differ in how a double is made from it: `resolution` 32 is THRandom_uniform's
// random() * 2^-32 (Torch7 up to 2017, the era of bot7), 53 the later ((random64() & (2^53 - 1)) * 2^-53 with
// random64 = (random() << 32) | random().  Sequential by construction, so it runs on the host (33M draws take 0.1 s) and
// only the affine map of grids/random.lua:27-33 runs on the device.
namespace {
struct Mt19937 {
  uint32_t mt[624];
  int idx;
  explicit Mt19937(uint32_t seed) {
    mt[0] = seed;
    for (int j = 1; j < 624; ++j) mt[j] = 1812433253u * (mt[j - 1] ^ (mt[j - 1] >> 30)) + (uint32_t)j;
    idx = 624;
  }
  uint32_t next() {
    if (idx >= 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
        mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      idx = 0;
    }
    uint32_t y = mt[idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};
}  // namespace

static int grid_random_torch_local(b7_ctx *c, int64_t size, int dims, uint64_t seed, int resolution, const double *mins,
                                   const double *maxes) {
  if (size < 0 || (resolution != 32 && resolution != 53))
    return b7_fail(c, B7_ERR_INVALID, "random grid (torch stream): size >= 0, resolution 32 or 53");
  std::vector<double> u((size_t)size * (dims > 0 ? dims : 0));
  if (dims >= 1 && b7_torch_rand(seed, (int64_t)u.size(), resolution, u.data()) != B7_OK)
    return b7_fail(c, B7_ERR_INVALID, "random grid (torch stream): bad arguments");
  B7_TRY(b7_grid_upload(c, u.data(), size, dims));
  if (mins && maxes && size > 0) {   // grids/random.lua:27-28: cmul by (maxes + -mins), then add mins: two rounded operations
    double *stage = c->pinned->vec, *v_dev = b7_scratch(c)->colvec;
    for (int pass = 0; pass < 2; ++pass) {
      B7_HIP(c, hipStreamSynchronize(c->stream));
      for (int k = 0; k < dims; ++k) stage[k] = pass == 0 ? maxes[k] + (-mins[k]) : mins[k];
      B7_HIP(c, hipMemcpyAsync(v_dev, stage, sizeof(double) * dims, hipMemcpyHostToDevice, c->stream));
      B7_TRY(launch_col_affine(c, cur_grid(c), c->M, dims, v_dev, pass == 0));
    }
  }
  return B7_OK;
}

extern "C" {

int b7_grid_sobol(b7_ctx *c, int64_t size, int dims, int64_t skip, const double *mins, const double *maxes,
                  double *out_host) {
  if (!c) return B7_ERR_INVALID;
  int rc = grid_sobol_local(c, size, dims, skip, mins, maxes);
  if ((mins != nullptr) != (maxes != nullptr)) rc = onesided(c, mins, maxes, rc);  // collective with a communicator: entered on failure too
  B7_TRY(rc);
  return grid_copy_out(c, out_host);
}

int b7_grid_random(b7_ctx *c, int64_t size, int dims, uint64_t seed, int64_t row_offset, const double *mins,
                   const double *maxes, double *out_host) {
  if (!c) return B7_ERR_INVALID;
  int rc = grid_random_local(c, size, dims, seed, row_offset, mins, maxes);
  if ((mins != nullptr) != (maxes != nullptr)) rc = onesided(c, mins, maxes, rc);
  B7_TRY(rc);
  return grid_copy_out(c, out_host);
}

int b7_torch_rand(uint64_t seed, int64_t n, int resolution, double *out) {
  if (n < 0 || (n > 0 && !out) || (resolution != 32 && resolution != 53)) return B7_ERR_INVALID;
  Mt19937 g((uint32_t)seed);
  if (resolution == 32)
    for (int64_t i = 0; i < n; ++i) out[i] = (double)g.next() * (1.0 / 4294967296.0);
  else
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t hi = g.next(), lo = g.next();
      out[i] = (double)(((hi << 32) | lo) & ((1ull << 53) - 1)) * 1.1102230246251565404e-16;
    }
  return B7_OK;
}

int b7_grid_random_torch(b7_ctx *c, int64_t size, int dims, uint64_t seed, int resolution, const double *mins,
                         const double *maxes, double *out_host) {
  if (!c) return B7_ERR_INVALID;
  int rc = grid_random_torch_local(c, size, dims, seed, resolution, mins, maxes);
  if ((mins != nullptr) != (maxes != nullptr)) rc = onesided(c, mins, maxes, rc);  // collective with a communicator: entered on failure too
  B7_TRY(rc);
  return grid_copy_out(c, out_host);
}

int b7_grid_colrange(b7_ctx *c, double *col_min, double *col_max) {
  if (!c) return B7_ERR_INVALID;
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "grid_colrange: no candidate grid on this context");
  B7_HIP(c, hipSetDevice(c->device));
  const int d = c->d;
  double *out_dev = b7_scratch(c)->colvec;
  B7_TRY(launch_colrange(c, cur_grid(c), c->M, d, out_dev));
  std::vector<double> h(2 * (size_t)d);
  B7_HIP(c, hipMemcpyAsync(h.data(), out_dev, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (col_min) memcpy(col_min, h.data(), sizeof(double) * d);
  if (col_max) memcpy(col_max, h.data() + d, sizeof(double) * d);
  return B7_OK;
}

int b7_grid_apply_onesided(b7_ctx *c, const double *mins, const double *maxes, const double *col_ext) {
  if (!c) return B7_ERR_INVALID;
  if ((mins != nullptr) == (maxes != nullptr) || !col_ext)
    return b7_fail(c, B7_ERR_INVALID, "grid_apply_onesided: exactly one of mins / maxes, and the column extremes");
  B7_TRY(group_guard(c, "grid_apply_onesided"));
  B7_HIP(c, hipSetDevice(c->device));
  const int d = c->d;
  // torch.add(mins, grid:min(1)[1]) (grids/sobol.lua:83) / torch.cdiv(maxes, grid:max(1)[1]) (:85): one rounded operation per
  // column, here; then one per element on the device
  double *stage = c->pinned->vec, *v_dev = b7_scratch(c)->colvec;
  B7_HIP(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < d; ++k) stage[k] = mins ? mins[k] + col_ext[k] : maxes[k] / col_ext[k];
  B7_HIP(c, hipMemcpyAsync(v_dev, stage, sizeof(double) * d, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_col_affine(c, cur_grid(c), c->M, d, v_dev, maxes != nullptr));
  invalidate_predictions(c);
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_grid_trust_region(b7_ctx *c, const double *center, const double *lo, const double *hi, double prob, const double *shift,
                         uint64_t seed, int64_t row_offset) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(group_guard(c, "grid_trust_region"));
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "grid_trust_region: no candidate grid on this context");
  if (!center || !lo || !hi) return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: center, lo or hi is NULL");
  if (!(prob >= 0.0 && prob <= 1.0)) return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: prob %g outside [0, 1]", prob);
  if (row_offset < 0) return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: row_offset %lld is negative", (long long)row_offset);
  const int d = c->d;
  for (int k = 0; k < d; ++k) {
    if (!isfinite(center[k]) || !isfinite(lo[k]) || !isfinite(hi[k]) || (shift && !isfinite(shift[k])))
      return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: column %d has a non-finite entry", k);
    if (lo[k] > hi[k]) return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: column %d has lo %g > hi %g", k, lo[k], hi[k]);
    if (center[k] < lo[k] || center[k] > hi[k])
      return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: column %d has its center %g outside [%g, %g]", k, center[k], lo[k], hi[k]);
    if (shift && !(shift[k] >= 0.0 && shift[k] < 1.0))
      return b7_fail(c, B7_ERR_INVALID, "grid_trust_region: column %d has shift %g outside [0, 1)", k, shift[k]);
  }
  B7_HIP(c, hipSetDevice(c->device));
  double *stage = c->pinned->tr, *v_dev = b7_scratch(c)->trvec;
  B7_HIP(c, hipStreamSynchronize(c->stream));  // nothing in flight reads the stage
  for (int k = 0; k < d; ++k) {
    stage[k] = center[k];
    stage[d + k] = lo[k];
    stage[2 * d + k] = hi[k] + (-lo[k]);  // the span as random_grid_kernel forms it
    stage[3 * d + k] = shift ? shift[k] : 0.0;
    stage[4 * d + k] = hi[k];
  }
  B7_HIP(c, hipMemcpyAsync(v_dev, stage, sizeof(double) * 5 * d, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_trust_region(c, cur_grid(c), c->M, d, v_dev, shift != nullptr, prob, seed, row_offset));
  invalidate_predictions(c);
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_grid_upload(b7_ctx *c, const double *X, int64_t M, int d) {
  if (!c) return B7_ERR_INVALID;
  if (!X && M > 0) return b7_fail(c, B7_ERR_INVALID, "grid_upload: X is NULL");
  B7_TRY(grid_alloc(c, M, d));
  if (M > 0)
    B7_HIP(c, hipMemcpyAsync(cur_grid(c), X, sizeof(double) * (size_t)M * d, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_grid_download(b7_ctx *c, int64_t row0, int64_t rows, double *out_host) {
  if (!c) return B7_ERR_INVALID;
  if (row0 < 0 || rows < 0 || row0 + rows > c->M || (!out_host && rows > 0))
    return b7_fail(c, B7_ERR_INVALID, "grid_download: rows [%lld, %lld) outside [0, %lld)", (long long)row0,
                   (long long)(row0 + rows), (long long)c->M);
  if (rows > 0)
    B7_HIP(c, hipMemcpyAsync(out_host, cur_grid(c) + row0 * c->d, sizeof(double) * (size_t)rows * c->d,
                             hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_grid_shape(b7_ctx *c, int64_t *M, int *d) {
  if (!c) return B7_ERR_INVALID;
  if (M) *M = c->M;
  if (d) *d = c->d;
  return B7_OK;
}

int b7_grid_remove(b7_ctx *c, int64_t idx1, double *row_out) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(grid_drop_row(c, idx1, row_out));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_grid_remove_rows(b7_ctx *c, const int64_t *idx1, int64_t n, double *rows_out) {
  if (!c) return B7_ERR_INVALID;
  if (n < 0 || (n > 0 && !idx1)) return b7_fail(c, B7_ERR_INVALID, "grid_remove_rows: bad index list");
  B7_TRY(group_guard(c, "grid_remove_rows"));
  if (n == 0) return B7_OK;
  for (int64_t i = 0; i < n; ++i)
    if (idx1[i] < 1 || idx1[i] > c->M)
      return b7_fail(c, B7_ERR_INVALID, "grid_remove_rows: index %lld outside [1, %lld]", (long long)idx1[i],
                     (long long)c->M);
  B7_HIP(c, hipSetDevice(c->device));
  // keep:indexFill(1, idx, 0) is idempotent: duplicates remove the row once (utils/tensor.lua:162)
  std::vector<int64_t> idx0(idx1, idx1 + n), cuts(idx1, idx1 + n);
  for (int64_t &v : idx0) v -= 1;
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
  const int64_t ncut = (int64_t)cuts.size();
  for (int64_t i = 0; i < ncut; ++i) cuts[i] = (cuts[i] - 1) - i;
  B7_TRY(b7_ensure(c, c->tmpvar, sizeof(int64_t) * (size_t)(n + ncut)));
  int64_t *idx0_dev = (int64_t *)c->tmpvar.p, *cuts_dev = idx0_dev + n;
  B7_HIP(c, hipMemcpyAsync(idx0_dev, idx0.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(cuts_dev, cuts.data(), sizeof(int64_t) * ncut, hipMemcpyHostToDevice, c->stream));
  if (rows_out) {
    B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (size_t)n * c->d));
    B7_TRY(launch_gather_rows(c, cur_grid(c), (double *)c->tmpmu.p, idx0_dev, n, c->d));
    B7_HIP(c, hipMemcpyAsync(rows_out, c->tmpmu.p, sizeof(double) * (size_t)n * c->d, hipMemcpyDeviceToHost, c->stream));
  }
  const int other = c->grid_cur ^ 1;
  B7_TRY(b7_ensure(c, c->grid[other], sizeof(double) * (size_t)c->M * c->d));
  B7_TRY(launch_remove_rows(c, cur_grid(c), (double *)c->grid[other].p, c->M, c->d, cuts_dev, (int)ncut));
  c->grid_cur = other;
  c->M -= ncut;
  invalidate_predictions(c);
  B7_HIP(c, hipStreamSynchronize(c->stream));  // idx0 / cuts (pageable) are consumed, rows_out is complete
  return B7_OK;
}

}  // extern "C"

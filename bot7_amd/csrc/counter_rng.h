// The library's counter-based generator: splitmix64 -> Box-Muller.  A draw is a pure function of (seed, counter), so any thread
// can produce any element of a stream and a stream does not depend on how many elements were asked for.
//
// Users and their counter layouts:
//   b7_gp_fantasize (extras.hip)   z(k, s) = counter_normal(seed, k * n + s): pending point k, draw s of n.
//   b7_ts_nominate  (rff.hip)      key(seed, a) = splitmix64(splitmix64(seed) ^ a) opens stream a of a call's seed:
//       a = 0        the random-feature BASIS, shared by the paths of a call; feature f owns the counters 128 f .. 128 f + 127:
//                      128 f + k        (k < 96)  z[f][k]  ~ N(0,1), the direction of Omega[f][k] before the lengthscales
//                      128 f + 96 + i   (i < 5)   g[f][i]  ~ N(0,1), u_f = sum g^2: the chi-square(5) of the Matern-5/2 spectrum
//                      128 f + 101                phase[f] = 2 pi counter_uniform
//       a = 1 + j    PATH j:   f (f < 4096)  weight[f] ~ N(0,1);   4096 + i  eps[i] / sqrt(noise) ~ N(0,1), observation i
//     Nothing depends on q, S, F, d or N: feature f, path j and observation i have the same draws in every call with that seed.
//   b7_blr_ts_nominate (blr_ts.hip)   PATH j draws from the stream key(seed, 2^32 + j), apart from every stream above:
//       k (k < 256)  eps_j[k] ~ N(0,1), component k of the weight draw.  A function of (seed, j, k) alone: not of q, S, z or N.
//   b7_gp_slice_sample (gp_small.hip: slice_chain_kernel)   chain c of a call draws from the stream key(seed, c); update number
//       g = update0 + u owns the counters 4096 g .. 4096 g + 4095 (D = d + 3 <= 64 components, at most 3840 shrink steps):
//                      4096 g + k        (k < D)     z_k ~ N(0,1), the direction before it is normalised (counter_normal)
//                      4096 g + 64                   u_Y: the slice level is f(x0) + log(u_Y)               (counter_uniform)
//                      4096 g + 128 + k  (k < D)     the uniform of right_k
//                      4096 g + 256 + i  (i < 3840)  the uniform of shrink step i
//     Nothing depends on C, U or how a run is split into calls: a draw is a function of (seed, chain, g).
//   b7_grid_trust_region (trust_region.hip: trust_region_kernel)   g = row_offset + i is a row's GLOBAL number, d the grid's dims:
//       key(seed, 0)   counter g d + k   the uniform of the mask of element (g, k): perturbed iff it is < prob        (counter_uniform)
//       key(seed, 1)   counter g         the uniform u of the row's forced column f(g) = min(d - 1, (int)(u d))       (counter_uniform)
//     Nothing depends on M or on how rows are split between calls: an element is a function of (seed, g, k).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// z(k, s) ~ N(0,1): Box-Muller on two counter-based uniforms; u1 in (0, 1]
__device__ inline double counter_normal(uint64_t seed, uint64_t ctr) {
  const uint64_t a = splitmix64(seed + 0x9E3779B97F4A7C15ull * (2 * ctr + 1));
  const uint64_t b = splitmix64(seed + 0x9E3779B97F4A7C15ull * (2 * ctr + 2));
  const double u1 = (double)((a >> 11) + 1) * 1.1102230246251565404e-16;
  const double u2 = (double)(b >> 11) * 1.1102230246251565404e-16;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
}
// u ~ U[0, 1): the first of the two uniforms counter_normal would take at this counter
__device__ inline double counter_uniform(uint64_t seed, uint64_t ctr) {
  const uint64_t a = splitmix64(seed + 0x9E3779B97F4A7C15ull * (2 * ctr + 1));
  return (double)(a >> 11) * 1.1102230246251565404e-16;
}
__host__ __device__ inline uint64_t counter_key(uint64_t seed, uint64_t stream) { return splitmix64(splitmix64(seed) ^ stream); }

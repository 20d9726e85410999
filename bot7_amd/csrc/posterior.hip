// Posterior variance over a chunk of candidates:  var_j = amp - || L^-1 k*_j ||^2.
//
// Reference arithmetic replaced: the variance half of model:predict(X_obs, Y_obs, X_hid, hyp, {mean, var})
// (call sites scores/expected_improvement.lua:63, scores/confidence_bound.lua:63; gp_regressor itself is in
// the absent `gp` package): textbook GP regression, V = L^-1 K(X*,X)', var = k** - colsumsq(V).
//
// This is the dominant kernel of the whole path: M * N^2 flops (4.19 MFLOP per candidate at N = 2048), all
// of it on v_mfma_f64_16x16x4_f64.  V is never stored: a workgroup owns 256 (large grids) or 128 (small grids)
// candidates, walks the 128-row tiles of the explicit inverse factor top to bottom (k only up to the diagonal: Linv
// is lower triangular) and folds each finished tile of V into per-candidate sums of squares held in registers.
//
// The arithmetic is fixed, and stated so that a host model can reproduce it bit for bit (tools/post_probe.hip does):
//   v[n][c]  = fma chain over k ascending of Linv[n][k] * K*[c][k]     (what a chain of v_mfma_f64_16x16x4_f64 computes,
//              tools/mfma_acc_probe.hip)
//   per lane group g = 0..3, 128-row tile t and row half h:  s = fma chain of v^2 over rows 16 I + g + 4 r  (I in the
//              half ascending, r ascending), colss[h] += s over t ascending
//   ss[c]    = ((g0 + g1) + (g2 + g3))_{h=0} + (...)_{h=1}
// so results do not depend on the grid size, the shard layout or the run -- the arg-max downstream relies on that.
//
// Shape history (N = 2048, 262144 candidates per launch, one MI355X): round 1, compiler-scheduled GEMM tile loop,
// 128 x 128 tile 44.6 TF -> 2 blocks/CU 59.2 -> odd LDS stride, zero-strip skip 61.6 -> 128 x 256 tile with 8 waves and
// a static priority raise 64.7 TF.  Round 2: in-kernel stamps (tools/post_clock.py: s_memtime / s_memrealtime around
// every workgroup after >= 2 s of back-to-back launches) showed the chip holding 2.37 GHz -- not the 2.1 GHz round 1
// had inferred from counters -- and the workgroup NOT issuing MFMAs for 14 % of its cycles: the two waves of a SIMD
// run in lock step, sit in the same LDS wait at mid-stage and at the barrier, and 256 registers per wave leave no room
// to fetch fragments ahead.  The kernels below: 96 % issue efficiency at 2.31-2.33 GHz, 71.7 TF (128-row n-tiles) and
// 73 TF (256-row n-tiles) = 91-93 % of the 78.6 TF peak.  The 256-row shape has since been given LDS-DMA staging into a ring
// of three images (its header below): 98.5 % issue efficiency, 2.5 % fewer cycles at the same clock.
//
// Algorithmic work per launch: rows * Npad^2 flops (triangle exploited), bytes: the K* chunk is read
// (t+1)/T-weighted ~ (T+1)/2 times from L2/MALL/HBM (T = Npad/128 n-tiles), Linv once per workgroup from L2.
#include "b7_internal.h"
#include "post_ring_layout.h"
#include <utility>

#ifdef B7_POST_STAMPS
// Diagnostic build only (tools/post_clock.py; never defined for the shipped library): every workgroup records
// s_memtime / s_memrealtime at its start and end into a buffer nothing else reads; the in-kernel clock is
// d(s_memtime) / d(s_memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS give-back item 6).
__device__ unsigned long long b7_post_stamps[4 * 4096];
extern "C" int b7dbg_post_stamps(unsigned long long *out, int nblocks) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(b7_post_stamps), sizeof(unsigned long long) * 4 * nblocks);
}
#endif

typedef double d2_t __attribute__((ext_vector_type(2)));

// Several fits over the same candidates in one launch (b7_eval_nominate: the hyper samples of a nomination): grid.y = fit;
// L^-1, K* and the output are strided per fit, amp (and the noise term when the variance includes it) come from arrays.
// base == nullptr: a single fit, the scalar arguments apply.
struct PostBatch {
  int64_t sLinv = 0, sks = 0, svar = 0;
  const double *base = nullptr, *var_add = nullptr;
};

// ---- one wave per SIMD, one continuous MFMA stream -----------------------------------------------------------------------
// Four waves (512 registers each); a wave owns all 128 rows of the n-tile and 16 NJ candidates: 8 x NJ accumulator
// tiles of 16 x 16 (NJ = 4: 128 x 256 workgroup tile; NJ = 2: 128 x 128, for grids with fewer than one 256-candidate
// workgroup per CU).  LDS image of a stage: [128 + 64 NJ][16 + 1] doubles (odd row stride: ds_read2_b64 fragment
// reads are conflict-free), two buffers.  A wave keeps two fragment sets and the next stage's global data in flight:
//   first half of stage n  : MFMAs of k-steps 0,1 (set F0) | read F1 = k-steps 2,3 of stage n | store G (stage n+1,
//                            loaded a stage ago) into the other LDS buffer | issue the global loads of stage n+2
//   barrier (mid-stage)    : stage n+1's image is complete; nobody reads this stage's buffer any more
//   second half of stage n : MFMAs of k-steps 2,3 (set F1) | read F0 = k-steps 0,1 of stage n+1
// The side operations are placed between the MFMAs in program order (about one every second MFMA), so a wave never
// waits on LDS or on memory, only on the barrier's skew.  The stage stream runs across the n-tiles without a
// prologue per tile; in the 8 diagonal stages of a tile the 16-row strips above the diagonal are skipped.  Two LDS
// buffers suffice: every read of a buffer precedes the mid-stage barrier of the stage after the one that computes from
// it, every write to it follows that barrier.
namespace w4 {
constexpr int BM = 128, BK = 16, LD = BK + 1, A_DBL = BM * LD;

// The accumulator tiles of a wave are AGPRs addressed by NUMBER inside inline asm, never held in a C++ variable:
// tile (i, j) is a[8 (NJ i + j) : 8 (NJ i + j) + 7].  (As compiler-visible values -- the builtin, or "+a" asm
// operands -- the register allocator carried some of them across the loop back-edge in VGPRs: hundreds of v_accvgpr
// copies per stage, spills, and no hazard handling after an asm MFMA.)  Every asm statement below names all 256 AGPRs as
// clobbered, so the compiler keeps nothing of its own in them; bot7_amd/build.py checks in the ISA of every build that no
// instruction outside these asm statements names an AGPR.
#define B7_W4_ACC_REGS \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", \
  "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", \
  "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", \
  "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", \
  "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", \
  "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", \
  "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", \
  "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", \
  "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", \
  "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", \
  "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", \
  "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", \
  "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", \
  "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", \
  "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", \
  "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", \
  "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", \
  "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", \
  "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"

template <int NJ, int I, int J, bool ZERO>
__device__ __forceinline__ void mfma_tile(double a, double b) {
  constexpr int lo = 8 * (NJ * I + J);
  if constexpr (ZERO)
    asm volatile("v_mfma_f64_16x16x4_f64 a[%2:%3], %0, %1, 0" ::"v"(a), "v"(b), "n"(lo), "n"(lo + 7) : B7_W4_ACC_REGS);
  else
    asm volatile("v_mfma_f64_16x16x4_f64 a[%2:%3], %0, %1, a[%2:%3]" ::"v"(a), "v"(b), "n"(lo), "n"(lo + 7)
                 : B7_W4_ACC_REGS);
}

// accumulator tile (I, J) back into VGPRs: the caller has drained the matrix pipe (s_nop) before the first one
template <int NJ, int I, int J>
__device__ __forceinline__ void read_tile(double (&v)[4]) {
  constexpr int lo = 8 * (NJ * I + J);
  unsigned w[8];
  asm volatile(
      "v_accvgpr_read_b32 %0, a[%8]\n\tv_accvgpr_read_b32 %1, a[%9]\n\tv_accvgpr_read_b32 %2, a[%10]\n\t"
      "v_accvgpr_read_b32 %3, a[%11]\n\tv_accvgpr_read_b32 %4, a[%12]\n\tv_accvgpr_read_b32 %5, a[%13]\n\t"
      "v_accvgpr_read_b32 %6, a[%14]\n\tv_accvgpr_read_b32 %7, a[%15]"
      : "=v"(w[0]), "=v"(w[1]), "=v"(w[2]), "=v"(w[3]), "=v"(w[4]), "=v"(w[5]), "=v"(w[6]), "=v"(w[7])
      : "n"(lo), "n"(lo + 1), "n"(lo + 2), "n"(lo + 3), "n"(lo + 4), "n"(lo + 5), "n"(lo + 6), "n"(lo + 7));
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = __hiloint2double((int)w[2 * r + 1], (int)w[2 * r]);
}

template <int NJ>
struct Frags {
  double a[2][8], b[2][NJ];  // two k-steps: 8 strips of L^-1 rows, NJ strips of candidates
};
template <int NJ>
struct Stage {  // global data of one stage in flight: 4 + 2 NJ sixteen-byte chunks per thread
  d2_t c[4 + 2 * NJ];
};
struct Cursor {  // (n-tile, 16-deep k block) of a stage; clamps at the last stage
  int t, kb, ntiles;
  __device__ __forceinline__ void advance() {
    if (kb + 1 < (t + 1) * (BM / BK)) {
      ++kb;
    } else if (t + 1 < ntiles) {
      ++t;
      kb = 0;
    }
  }
};

template <int N, class F, int... Is>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl<N>(f, std::make_integer_sequence<int, N>{});
}

// fragment pair P of a two-k-step set: P < NJ candidates strip P, else rows strip P - NJ (k-steps S0, S0 + 1)
template <int NJ, int P, int S0>
__device__ __forceinline__ void read_pair(Frags<NJ> &f, const double *__restrict__ sa, const double *__restrict__ sb) {
  if constexpr (P < NJ) {
    f.b[0][P] = sb[P * 16 * LD + 4 * S0];
    f.b[1][P] = sb[P * 16 * LD + 4 * S0 + 4];
  } else {
    f.a[0][P - NJ] = sa[(P - NJ) * 16 * LD + 4 * S0];
    f.a[1][P - NJ] = sa[(P - NJ) * 16 * LD + 4 * S0 + 4];
  }
}

// chunk C of a stage: C < 4 rows r0 + 32 C of the L^-1 tile, else candidates r0 + 32 (C - 4) of the K* tile
template <int NJ, int C>
__device__ __forceinline__ void load_chunk(Stage<NJ> &g, const double *__restrict__ qa, const double *__restrict__ qb,
                                           int64_t lda) {
  if constexpr (C < 4)
    g.c[C] = *reinterpret_cast<const d2_t *>(qa + (int64_t)(32 * C) * lda);
  else
    g.c[C] = *reinterpret_cast<const d2_t *>(qb + (int64_t)(32 * (C - 4)) * lda);
}
template <int NJ, int C>
__device__ __forceinline__ void store_chunk(const Stage<NJ> &g, double *__restrict__ w) {
  constexpr int o = C < 4 ? 32 * C * LD : A_DBL + 32 * (C - 4) * LD;
  w[o] = g.c[C][0];
  w[o + 1] = g.c[C][1];
}

// One stage of the stream.  FIRST = first 16-row strip with anything to do (0 away from the diagonal block); ZERO: the
// first stage of an n-tile starts the accumulators from the literal 0.  NM MFMAs per half; the side operations of a half
// (first: the fragment pairs of F1, the LDS stores of the next stage, the global loads of the one after; second: the
// fragment pairs of the next stage's F0) are spread evenly between them.
template <int NJ, int FIRST, bool ZERO>
__device__ __forceinline__ void stage(Frags<NJ> &f0, Frags<NJ> &f1, Stage<NJ> &g, double *__restrict__ cur,
                                      double *__restrict__ nxt, int fa, int fb, int wofs, const double *__restrict__ pa,
                                      const double *__restrict__ pb, int64_t lda, Cursor &ld) {
  constexpr int NI = 8 - FIRST, NM = 2 * NJ * NI, NP = 8 + NJ, NC = 4 + 2 * NJ, NS = NP + 2 * NC;
  const double *qa = pa + ((int64_t)ld.t * BM) * lda + ld.kb * BK, *qb = pb + ld.kb * BK;
  ld.advance();
  // ---- first half: k-steps 0, 1 from F0
  constexpr int K1 = (NS + NM - 1) / NM + 1, K2 = (NP + NM - 1) / NM + 1;  // side operations behind one MFMA, at most
  static_for<NM>([&](auto m_) {
    constexpr int m = decltype(m_)::value, ks = m / (NJ * NI), i = FIRST + (m % (NJ * NI)) / NJ, j = m % NJ;
    mfma_tile<NJ, i, j, ZERO && ks == 0>(f0.a[ks][i], f0.b[ks][j]);
    static_for<K1>([&](auto k_) {
      constexpr int sidx = m * NS / NM + decltype(k_)::value;
      if constexpr (sidx < (m + 1) * NS / NM) {
        if constexpr (sidx < NP) {
          if constexpr (sidx < NJ || sidx - NJ >= FIRST) read_pair<NJ, sidx, 2>(f1, cur + fa, cur + fb);
        } else if constexpr (sidx < NP + NC) {
          store_chunk<NJ, sidx - NP>(g, nxt + wofs);
        } else {
          load_chunk<NJ, sidx - NP - NC>(g, qa, qb, lda);
        }
      }
    });
  });
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's part of the next image is in LDS (the loads stay in flight)
  __builtin_amdgcn_s_barrier();
  // ---- second half: k-steps 2, 3 from F1; the next stage's F0 (all strips: its FIRST is not known here)
  static_for<NM>([&](auto m_) {
    constexpr int m = decltype(m_)::value, ks = m / (NJ * NI), i = FIRST + (m % (NJ * NI)) / NJ, j = m % NJ;
    mfma_tile<NJ, i, j, false>(f1.a[ks][i], f1.b[ks][j]);
    static_for<K2>([&](auto k_) {
      constexpr int sidx = m * NP / NM + decltype(k_)::value;
      if constexpr (sidx < (m + 1) * NP / NM) read_pair<NJ, sidx, 0>(f0, nxt + fa, nxt + fb);
    });
  });
}

template <int NJ>
__global__ void __launch_bounds__(256)
    post_kernel_w4(const double *__restrict__ Linv, const double *__restrict__ ks, int Npad, int64_t row0, int64_t Mtotal,
                   double base, double sgn, double var_add, int clamp, double var_min, double *__restrict__ var,
                   PostBatch bat) {
  constexpr int BN = 64 * NJ, STAGE_DBL = (BM + BN) * LD, NC = 4 + 2 * NJ, NP = 8 + NJ;
  extern __shared__ __align__(16) double sm[];
  if (bat.base) {
    const int64_t y = blockIdx.y;
    Linv += y * bat.sLinv;
    ks += y * bat.sks;
    var += y * bat.svar;
    base = bat.base[y];
    if (bat.var_add) var_add = bat.var_add[y];
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef B7_POST_STAMPS
  const unsigned long long st0 = __builtin_amdgcn_s_memtime(), sr0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  const int64_t lda = Npad;
  // staging: thread -> (row r0 + 32 i, 16-byte chunk kc) of both operand tiles
  const int r0 = threadIdx.x >> 3, kc = threadIdx.x & 7;
  const double *pa = Linv + (int64_t)r0 * lda + 2 * kc;
  const double *pb = ks + ((int64_t)blockIdx.x * BN + r0) * lda + 2 * kc;
  const int wofs = r0 * LD + 2 * kc;
  // fragments: lane -> (row or candidate lane & 15 of a strip, k = 4 s + (lane >> 4))
  const int fa = (lane & 15) * LD + (lane >> 4);
  const int fb = A_DBL + (wave * 16 * NJ + (lane & 15)) * LD + (lane >> 4);

  const int ntiles = Npad / BM;
  Cursor ld{0, 0, ntiles};
  Stage<NJ> g;
  Frags<NJ> f0, f1;
  double *const b0 = sm, *const b1 = sm + STAGE_DBL;  // every tile has an even number of stages: it starts on b0
  static_for<NC>([&](auto c_) { load_chunk<NJ, decltype(c_)::value>(g, pa, pb, lda); });  // stage 0
  ld.advance();
  static_for<NC>([&](auto c_) { store_chunk<NJ, decltype(c_)::value>(g, b0 + wofs); });
  {
    const double *qa = pa + ((int64_t)ld.t * BM) * lda + ld.kb * BK, *qb = pb + ld.kb * BK;
    static_for<NC>([&](auto c_) { load_chunk<NJ, decltype(c_)::value>(g, qa, qb, lda); });  // stage 1: stored during stage 0
    ld.advance();
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  static_for<NP>([&](auto p_) { read_pair<NJ, decltype(p_)::value, 0>(f0, b0 + fa, b0 + fb); });

  double colss[2][NJ] = {};  // rows 0..63 and 64..127 of every n-tile apart
#define B7_STAGE(F, Z, CUR, NXT) stage<NJ, F, Z>(f0, f1, g, CUR, NXT, fa, fb, wofs, pa, pb, lda, ld)
  for (int t = 0; t < ntiles; ++t) {
    // 8 t stages away from the diagonal block, then its 8 stages (in stage q the strips 0..q-1 hold zeros only); the
    // tile's first stage starts the accumulators from zero; buffers alternate, b0 first
    B7_STAGE(0, true, b0, b1);
    if (t > 0) {
      for (int p = 0; p < 4 * t - 1; ++p) {
        B7_STAGE(0, false, b1, b0);
        B7_STAGE(0, false, b0, b1);
      }
      B7_STAGE(0, false, b1, b0);
      B7_STAGE(0, false, b0, b1);
    }
    B7_STAGE(1, false, b1, b0);
    B7_STAGE(2, false, b0, b1);
    B7_STAGE(3, false, b1, b0);
    B7_STAGE(4, false, b0, b1);
    B7_STAGE(5, false, b1, b0);
    B7_STAGE(6, false, b0, b1);
    B7_STAGE(7, false, b1, b0);
    // the asm MFMAs are opaque to the compiler's hazard recogniser: drain the matrix pipe before VALU reads the tile
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    static_for<2 * NJ>([&](auto hj_) {
      constexpr int h = decltype(hj_)::value / NJ, j = decltype(hj_)::value % NJ;
      double s = 0.0;
      static_for<4>([&](auto i_) {
        double v[4];
        read_tile<NJ, 4 * h + decltype(i_)::value, j>(v);
#pragma unroll
        for (int r = 0; r < 4; ++r) s = __builtin_fma(v[r], v[r], s);  // explicit: the order is part of the result
      });
      colss[h][j] += s;
    });
  }
#undef B7_STAGE

  // lanes l, l^16, l^32, l^48 hold partial sums of the same candidate; then the two row halves
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    double v0 = colss[0][j], v1 = colss[1][j];
    v0 += __shfl_xor(v0, 16);
    v0 += __shfl_xor(v0, 32);
    v1 += __shfl_xor(v1, 16);
    v1 += __shfl_xor(v1, 32);
    const int64_t gidx = row0 + (int64_t)blockIdx.x * BN + wave * 16 * NJ + j * 16 + lane;
    if (lane < 16 && gidx < Mtotal) {
      double ss = v0;
      ss += v1;
      double v = (base + sgn * ss) + var_add;  // GP: amp - ss; Bayesian-linear head: 1/beta + ss
      if (clamp) v = (v < var_min) ? var_min : v;  // TH clamp: NaN passes through
      var[gidx] = v;
    }
  }
#ifdef B7_POST_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < 4096) {
    const unsigned long long st1 = __builtin_amdgcn_s_memtime(), sr1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    unsigned long long *o = b7_post_stamps + 4 * blockIdx.x;
    o[0] = st0, o[1] = sr0, o[2] = st1, o[3] = sr1;
  }
#endif
}

template <int NJ>
constexpr int lds_bytes() { return 2 * (BM + 64 * NJ) * LD * 8; }

// ---- the tall shape: 256 rows of L^-1 x 128 candidates per workgroup ------------------------------------------------------
// Same stream, same 32 accumulator tiles per wave (16 strips of rows x 2 strips of candidates), but an n-tile of 256 rows:
// the K* rows of a workgroup are walked Npad/256 times instead of Npad/128, which halves the K* bytes the kernel pulls
// through the L2 (the traffic the counters price at 8.6x the algorithmic bytes) at the price of reading L^-1 twice as
// often from the L2 it is resident in.  The fragment sets hold ONE k-step each and alternate per k-step.
//
// Operands reach LDS by LDS-DMA (global_load_lds_dwordx4), never through registers: a stage image is 384 rows at a
// 128-byte pitch, XOR-swizzled (post_ring_layout.h: the one map the DMA source addresses and the fragment reads share),
// 48 pieces of 1 KiB; a wave issues twelve of them per stage, M0 = the piece's LDS address, source = a scalar base
// (n-tile row, k block and the piece's row offset, advanced on the SALU) + ONE 32-bit per-lane offset that is constant
// for the whole kernel.  Three images form a ring:
//   k-step 0: MFMAs(set 0) | read set 1 = k-step 1 | DMA pieces 0..3 of stage n+2 into buffer (n+2) % 3
//   k-step 1: MFMAs(set 1) | read set 0 = k-step 2 | DMA pieces 4..7
//   k-step 2: MFMAs(set 0) | read set 1 = k-step 3 | DMA pieces 8..11; the last three MFMAs carry nothing
//   s_waitcnt vmcnt(12) lgkmcnt(0); s_barrier
//   k-step 3: MFMAs(set 1) | read set 0 = k-step 0 of stage n+1 from buffer (n+1) % 3
// (the pieces sit evenly between the reads).  Ring invariant.  RAW: a wave's pieces of stage n+1 were issued during stage
// n-1; vmcnt(12) in front of stage n's barrier leaves only the twelve of stage n+2 in flight (loads retire in order), so
// behind that barrier every wave's part of image n+1 is in LDS, and nothing reads it earlier.  WAR: buffer (n+2) % 3 =
// (n-1) % 3 was last read by stage n-1's fragment reads, all of them issued -- and, by lgkmcnt(0), returned -- in front of
// stage n-1's barrier; every DMA into it is issued behind that barrier.  Only s_barrier and s_waitcnt order anything: a slip
// here gives wrong bits, never a hang.  The pieces requested past the last stage (the cursor clamps) are waited for before
// the workgroup ends and its LDS goes to the next one.
// No VALU instruction is left in the stream: every LDS address a lane reads through (3 ring positions x 4 k-steps x 2
// operands, strips as immediates) sits in a register for the whole kernel, and the stages name their ring position at
// compile time, a tile starting at position 0.  A tile has 16 (t + 1) stages, not a multiple of three, so once or twice
// per tile Lane::rotate renames the buffers (24 register moves) instead.  (With one runtime base added per k-step and
// operand -- eight v_add_u32 per stage -- the kernel kept 1.5 % of its cycles: DESIGN section 8.)
// The fold runs over the two 128-row halves of the tile in the order of the 128-row kernels, so the bits are the same.
template <int NJ, int NR>
struct Tall {
  static constexpr int BMT = 16 * NR, BN = 64 * NJ, ROWS = BMT + BN;
  static constexpr int STAGE_BYTES = ROWS * post_ring::ROW_BYTES, NBUF = 3;
  static constexpr int ND = ROWS / post_ring::PIECE_ROWS / post_ring::WAVES;  // DMA pieces per wave and stage
  static constexpr int NDA = BMT / post_ring::PIECE_ROWS / post_ring::WAVES;  // of them L^-1 rows
  static constexpr int NP = NR + NJ;
  static constexpr int LDS_BYTES = NBUF * STAGE_BYTES;
  static_assert(NJ * NR == 32, "32 accumulator tiles per wave");
  static_assert(ND == 12 && ND % 3 == 0, "vmcnt(12) below is ND; a third of the pieces per k-step");
  static_assert(LDS_BYTES <= 160 * 1024, "three stage images in 160 KiB");

  struct Set {
    double a[NR], b[NJ];
  };
  typedef __attribute__((address_space(3))) double lds_double;  // fragment reads go through LDS ADDRESSES held in registers
  // per-lane constants: fragment byte addresses per ring position and k-step (L^-1 strips; candidates strips), the DMA
  // source offset; wave-uniform: the LDS address of the wave's first piece per ring position.  Ring positions are LOGICAL:
  // the stages of a tile name them at compile time, position 0 first, so that no address is formed inside the stream;
  // where the stream's stage count is not a multiple of three (once or twice per tile) rotate() renames the buffers.
  struct Lane {
    int fa[NBUF][4], fb[NBUF][4];
    unsigned src, dst[NBUF];
    __device__ __forceinline__ void rotate1() {  // position p becomes what p + 1 was
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int a = fa[0][s], b = fb[0][s];
        fa[0][s] = fa[1][s], fa[1][s] = fa[2][s], fa[2][s] = a;
        fb[0][s] = fb[1][s], fb[1][s] = fb[2][s], fb[2][s] = b;
      }
      const unsigned d = dst[0];
      dst[0] = dst[1], dst[1] = dst[2], dst[2] = d;
    }
    __device__ __forceinline__ void rotate(int k) {  // k wave-uniform
      if (k >= 1) rotate1();
      if (k >= 2) rotate1();
    }
  };
  struct Cursor {
    int t, kb, ntiles;
    __device__ __forceinline__ void advance() {
      if (kb + 1 < (t + 1) * (BMT / BK)) {
        ++kb;
      } else if (t + 1 < ntiles) {
        ++t;
        kb = 0;
      }
    }
  };

  // fragment P of k-step S from the image at ring position B: P < NJ candidates strip P, else rows strip P - NJ
  template <int P, int S, int B>
  static __device__ __forceinline__ void read_one(Set &f, const Lane &ln) {
    constexpr int strip = (P < NJ ? P : P - NJ) * 16 * post_ring::ROW_BYTES;
    if constexpr (P < NJ)
      f.b[P] = *reinterpret_cast<const lds_double *>((uintptr_t)(unsigned)(ln.fb[B][S] + strip));
    else
      f.a[P - NJ] = *reinterpret_cast<const lds_double *>((uintptr_t)(unsigned)(ln.fa[B][S] + strip));
  }
  // piece C of this wave: C < NDA rows 32 C + 8 wave .. + 7 of the L^-1 tile, else candidates 32 (C - NDA) + 8 wave .. + 7
  // (ga, gb: the wave's first piece of either operand; dst: LDS byte address of the wave's first piece in the image)
  template <int C>
  static __device__ __forceinline__ void dma_piece(const char *__restrict__ ga, const char *__restrict__ gb, int64_t step,
                                                   unsigned src, unsigned dst) {
    const char *g = C < NDA ? ga + C * step : gb + (C - NDA) * step;
    const unsigned m0 = dst + C * post_ring::WAVES * post_ring::PIECE_BYTES;
    // M0 is written in the statement that uses it (s_nop 0: SALU write of M0 -> LDS-DMA); nothing else in the kernel uses M0
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0), "v"(src), "s"(g) : "memory");
  }

  // one k-step: NJ * (NR - FIRST) MFMAs from set `use`, NSIDE side operations spread between all but the last TAIL of them
  template <int FIRST, bool ZERO, int NSIDE, int TAIL, class Side>
  static __device__ __forceinline__ void kstep(const Set &use, Side &&side) {
    constexpr int NI = NR - FIRST, NM = NJ * NI, NMS = NM > 2 * TAIL ? NM - TAIL : NM;
    constexpr int KMAX = (NSIDE + NMS - 1) / NMS + 1;  // side operations behind one MFMA: [m NSIDE / NMS, (m + 1) NSIDE / NMS)
    static_for<NM>([&](auto m_) {
      constexpr int m = decltype(m_)::value, i = FIRST + m / NJ, j = m % NJ;
      mfma_tile<NJ, i, j, ZERO>(use.a[i], use.b[j]);
      if constexpr (m < NMS)
        static_for<KMAX>([&](auto k_) {
          constexpr int sidx = m * NSIDE / NMS + decltype(k_)::value;
          if constexpr (sidx < (m + 1) * NSIDE / NMS) side(std::integral_constant<int, sidx>{});
        });
    });
  }
  // the side slots of a k-step that carries NP fragment reads and H DMA pieces: the pieces sit evenly between the reads
  static constexpr int H = ND / 3, NS = NP + H;
  static constexpr int dma_before(int x) {  // DMA slots among the slots below x
    int n = 0;
    for (int d = 0; d < H; ++d) n += (d + 1) * NS / (H + 1) < x;
    return n;
  }
  static constexpr bool is_dma(int x) { return dma_before(x + 1) > dma_before(x); }

  // FIRST / NEXT_FIRST: first strip with anything to do in this stage / in the next one.  POS: ring position of this
  // stage's image; the next one's is POS + 1, the DMA pieces of the one after go to POS + 2
  template <int FIRST, int NEXT_FIRST, bool ZERO, int POS>
  static __device__ __forceinline__ void stage(Set &s0, Set &s1, const Lane &ln,
                                               const char *__restrict__ pa, const char *__restrict__ pb, int64_t lda, Cursor &ld) {
    constexpr int CUR = POS % NBUF, NXT = (POS + 1) % NBUF, DST = (POS + 2) % NBUF;
    const int64_t step = 32 * lda * 8;
    const char *ga = pa + (((int64_t)ld.t * BMT) * lda + ld.kb * BK) * 8, *gb = pb + (int64_t)(ld.kb * BK) * 8;
    ld.advance();
    auto sides = [&](auto ks_, Set &into, auto x_) {  // k-step ks: read the set of k-step ks + 1, pieces H ks .. H ks + H - 1
      constexpr int ks = decltype(ks_)::value, x = decltype(x_)::value, r = x - dma_before(x);
      if constexpr (is_dma(x))
        dma_piece<H * ks + dma_before(x)>(ga, gb, step, ln.src, ln.dst[DST]);
      else if constexpr (r < NJ || r - NJ >= FIRST)
        read_one<r, ks + 1, CUR>(into, ln);
    };
    kstep<FIRST, ZERO, NS, 0>(s0, [&](auto x_) { sides(std::integral_constant<int, 0>{}, s1, x_); });
    kstep<FIRST, false, NS, 0>(s1, [&](auto x_) { sides(std::integral_constant<int, 1>{}, s0, x_); });
    // the last MFMAs in front of the barrier carry nothing: the reads are back when lgkmcnt(0) asks
    kstep<FIRST, false, NS, 3>(s0, [&](auto x_) { sides(std::integral_constant<int, 2>{}, s1, x_); });
    // this wave's pieces of the next image have landed (the twelve just issued stay in flight); its reads of this image are back
    asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    kstep<FIRST, false, NP, 0>(s1, [&](auto s_) {
      constexpr int x = decltype(s_)::value;
      if constexpr (x < NJ || x - NJ >= NEXT_FIRST) read_one<x, 0, NXT>(s0, ln);
    });
  }
};

template <int NJ, int NR>
__global__ void __launch_bounds__(256)
    post_kernel_w4t(const double *__restrict__ Linv, const double *__restrict__ ks, int Npad, int64_t row0, int64_t Mtotal,
                    double base, double sgn, double var_add, int clamp, double var_min, double *__restrict__ var,
                    PostBatch bat) {
  using T = Tall<NJ, NR>;
  constexpr int BMT = T::BMT, BN = T::BN, NP = T::NP;
  extern __shared__ __align__(16) double sm[];
  if (bat.base) {
    const int64_t y = blockIdx.y;
    Linv += y * bat.sLinv;
    ks += y * bat.sks;
    var += y * bat.svar;
    base = bat.base[y];
    if (bat.var_add) var_add = bat.var_add[y];
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef B7_POST_STAMPS
  const unsigned long long st0 = __builtin_amdgcn_s_memtime(), sr0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  const int64_t lda = Npad;
  // DMA: the wave's first piece of either operand (rows 8 wave .. + 7); a lane's source offset is the same for all its pieces
  const char *pa = reinterpret_cast<const char *>(Linv + (int64_t)(post_ring::PIECE_ROWS * wave) * lda);
  const char *pb = reinterpret_cast<const char *>(ks + ((int64_t)blockIdx.x * BN + post_ring::PIECE_ROWS * wave) * lda);
  typename T::Lane ln;
  {
    const post_ring::Chunk c = post_ring::dma_src(wave, lane);
    ln.src = (unsigned)(((c.row - post_ring::PIECE_ROWS * wave) * Npad + 2 * c.chunk) * 8);
  }
  // fragments: lane -> (row or candidate lane & 15 of a strip, k = 4 s + (lane >> 4)); the swizzle does not depend on the strip
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)sm;
#pragma unroll
  for (int b = 0; b < T::NBUF; ++b) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      ln.fa[b][s] = lds0 + b * T::STAGE_BYTES + post_ring::frag_byte(lane & 15, 4 * s + (lane >> 4));
      ln.fb[b][s] = ln.fa[b][s] + (BMT + wave * 16 * NJ) * post_ring::ROW_BYTES;
      asm volatile("" : "+v"(ln.fa[b][s]), "+v"(ln.fb[b][s]));  // registers, not sums formed again at every read
    }
    ln.dst[b] = lds0 + b * T::STAGE_BYTES + wave * post_ring::PIECE_BYTES;
  }

  const int ntiles = Npad / BMT;
  typename T::Cursor ld{0, 0, ntiles};
  typename T::Set s0, s1;
  {
    const int64_t step = 32 * lda * 8;
    static_for<T::ND>([&](auto c_) { T::template dma_piece<decltype(c_)::value>(pa, pb, step, ln.src, ln.dst[0]); });  // stage 0
    ld.advance();
    const char *ga = pa + (((int64_t)ld.t * BMT) * lda + ld.kb * BK) * 8, *gb = pb + (int64_t)(ld.kb * BK) * 8;
    static_for<T::ND>([&](auto c_) { T::template dma_piece<decltype(c_)::value>(ga, gb, step, ln.src, ln.dst[1]); });  // stage 1
    ld.advance();
  }
  asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // stage 0 has landed
  __builtin_amdgcn_s_barrier();
  static_for<NP>([&](auto p_) { T::template read_one<decltype(p_)::value, 0, 0>(s0, ln); });

  double colss[2][NJ] = {};
#define B7_STAGE(F, NF, Z, POS) T::template stage<F, NF, Z, POS>(s0, s1, ln, pa, pb, lda, ld)
  for (int t = 0; t < ntiles; ++t) {
    // a tile starts at ring position 0: the zeroing stage, 16 t - 1 more stages away from the diagonal block three at a
    // time, the block's 16 stages from position 0 again
    B7_STAGE(0, 0, true, 0);
    if (t > 0) {
      const int n = NR * t - 1;
      for (int p = 0; p < n / 3; ++p) {
        B7_STAGE(0, 0, false, 1);
        B7_STAGE(0, 0, false, 2);
        B7_STAGE(0, 0, false, 0);
      }
      if (n % 3 >= 1) B7_STAGE(0, 0, false, 1);
      if (n % 3 == 2) B7_STAGE(0, 0, false, 2);
      ln.rotate((n + 1) % 3);
      B7_STAGE(0, 1, false, 0);  // diagonal stage 0
    }
    // diagonal stages 1 .. NR-1 (for t == 0 the zeroing stage above was diagonal stage 0; it read the next set in full)
    static_for<NR - 1>([&](auto q_) {
      constexpr int Q = decltype(q_)::value + 1;
      B7_STAGE(Q, (Q + 1) % NR, false, Q % 3);
    });
    ln.rotate(NR % 3);  // the next tile's position 0
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    // the tile is NR/8 128-row tiles of the fold, each as (rows 0..63, rows 64..127), in ascending order
    static_for<(NR / 4) * NJ>([&](auto qj_) {
      constexpr int q = decltype(qj_)::value / NJ, j = decltype(qj_)::value % NJ;  // q: 64-row group of the tile
      double s = 0.0;
      static_for<4>([&](auto i_) {
        double v[4];
        read_tile<NJ, 4 * q + decltype(i_)::value, j>(v);
#pragma unroll
        for (int r = 0; r < 4; ++r) s = __builtin_fma(v[r], v[r], s);
      });
      colss[q & 1][j] += s;
    });
  }
#undef B7_STAGE
  // the pieces requested past the last stage (the cursor clamps there) land before the workgroup gives up its LDS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    double v0 = colss[0][j], v1 = colss[1][j];
    v0 += __shfl_xor(v0, 16);
    v0 += __shfl_xor(v0, 32);
    v1 += __shfl_xor(v1, 16);
    v1 += __shfl_xor(v1, 32);
    const int64_t gidx = row0 + (int64_t)blockIdx.x * BN + wave * 16 * NJ + j * 16 + lane;
    if (lane < 16 && gidx < Mtotal) {
      double ss = v0;
      ss += v1;
      double v = (base + sgn * ss) + var_add;
      if (clamp) v = (v < var_min) ? var_min : v;
      var[gidx] = v;
    }
  }
#ifdef B7_POST_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < 4096) {
    const unsigned long long st1 = __builtin_amdgcn_s_memtime(), sr1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    unsigned long long *o = b7_post_stamps + 4 * blockIdx.x;
    o[0] = st0, o[1] = sr0, o[2] = st1, o[3] = sr1;
  }
#endif
}
}  // namespace w4

// ---- one 64-block: N <= 64 observations (the first 64 trials of every run at the reference's defaults) or the 50 basis
// features of the DNGO head.  A persistent workgroup (two per CU) reads the A fragments of L^-1 (64 x 64) into registers once
// and walks tiles of 64 candidates -- their K* rows staged through LDS, the next tile's in flight meanwhile --, a wave 16 of
// them: v = L^-1 K*' as four accumulator tiles, every chain over k ascending up to the row tile's diagonal (what is above is
// zero), then per candidate the sum of squares over the 64 rows in a fixed order: per lane group g the fma chain over rows
// 16 I + g + 4 r (I, then r, ascending), ((g0 + g1) + (g2 + g3)).
// Nothing here depends on the grid size, the shard or the launch shape, as in the large kernels.
namespace small64 {
typedef double d4_t __attribute__((ext_vector_type(4)));
constexpr int NB = 64, LLD = NB + 2, BN = 64;  // 64 candidates per tile: ~200 registers, two workgroups per CU -- one loads while the other computes
constexpr int LDS_BYTES = BN * LLD * 8;  // the K* tile; L^-1 lives in registers

__global__ void __launch_bounds__(256)
    post_small_kernel(const double *__restrict__ Linv, const double *__restrict__ ks, int64_t row0, int64_t Mtotal, int ntiles,
                      double base, double sgn, double var_add, int clamp, double var_min, double *__restrict__ var, PostBatch bat) {
  extern __shared__ __align__(16) double sm[];
  if (bat.base) {
    const int64_t y = blockIdx.y;
    Linv += y * bat.sLinv;
    ks += y * bat.sks;
    var += y * bat.svar;
    base = bat.base[y];
    if (bat.var_add) var_add = bat.var_add[y];
  }
  double *Ks = sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  // a workgroup walks tiles blockIdx.x, + gridDim.x, ...; the K* rows of the NEXT tile are on their way (16 chunks of 16 bytes
  // per thread, a wave reading two whole 512-byte rows per instruction) while this one is computed
  d2_t pv[BN / 8];
  auto fetch = [&](int tile) {
    const double *kt = ks + ((int64_t)tile * BN) * NB;
#pragma unroll
    for (int i = 0; i < BN / 8; ++i) {
      const int e = tid + 256 * i;
      pv[i] = *reinterpret_cast<const d2_t *>(kt + (int64_t)(e >> 5) * NB + 2 * (e & 31));
    }
  };
  int tile = blockIdx.x;
  if (tile < ntiles) fetch(tile);
  // L^-1 is the same for every tile: its A fragments -- row tile I, k-steps 0 .. 4 I + 3 (nothing above the diagonal) -- are
  // read from memory ONCE into 40 registers per lane; per tile only the candidates' fragments come from LDS, sixteen per
  // candidate strip, and the MFMA chains run from registers
  double af[40];
#pragma unroll
  for (int I = 0; I < 4; ++I)
#pragma unroll
    for (int k4 = 0; k4 < 4 * (I + 1); ++k4) af[2 * I * (I + 1) + k4] = Linv[(int64_t)(I * 16 + lr) * NB + 4 * k4 + lq];
  // every load so far has landed before the loop is entered: with the 40 fragment loads still counted as outstanding at the
  // loop head, the compiler's (counter-based) waits for them sit in the middle of the MFMA section and, from the second
  // iteration on, wait for the PREFETCH instead -- load and compute times added up (41 us for 1564 tiles) instead of overlapping
  // (as empty asm statements that "use" the fragments: a plain s_waitcnt does not keep the optimiser from sinking the loads
  // below it, and only a wait the compiler inserted itself clears its bookkeeping)
#pragma unroll
  for (int g = 0; g < 4; ++g)
    asm volatile("" : "+v"(af[10 * g]), "+v"(af[10 * g + 1]), "+v"(af[10 * g + 2]), "+v"(af[10 * g + 3]), "+v"(af[10 * g + 4]),
                      "+v"(af[10 * g + 5]), "+v"(af[10 * g + 6]), "+v"(af[10 * g + 7]), "+v"(af[10 * g + 8]), "+v"(af[10 * g + 9]));
  for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < BN / 8; ++i) {
      const int e = tid + 256 * i, r = e >> 5, c2 = 2 * (e & 31);
      Ks[r * LLD + c2] = pv[i][0];
      Ks[r * LLD + c2 + 1] = pv[i][1];
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) fetch(tile + gridDim.x);
    __builtin_amdgcn_sched_barrier(0);  // the loads go out HERE: left to itself the scheduler sinks them below the MFMA section
                                        // to shorten 64 registers' live range, and load and compute times add instead of overlapping
    constexpr int NJ = BN / 64;  // 16-candidate strips per wave
    double ss[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const double *bp = Ks + (wave * 16 * NJ + j * 16 + lr) * LLD + lq;
      double bf[16];
#pragma unroll
      for (int k4 = 0; k4 < 16; ++k4) bf[k4] = bp[4 * k4];
      double s = 0.0;
#pragma unroll
      for (int I = 0; I < 4; ++I) {
        d4_t c = {0.0, 0.0, 0.0, 0.0};
#ifdef B7_PS_ABLATE  // diagnostic build only (never defined for the shipped library): one MFMA per chain instead of 4 (I + 1)
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(af[2 * I * (I + 1)], bf[I], c, 0, 0, 0);
#else
#pragma unroll
        for (int k4 = 0; k4 < 4 * (I + 1); ++k4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(af[2 * I * (I + 1) + k4], bf[k4], c, 0, 0, 0);
#endif
#pragma unroll
        for (int r = 0; r < 4; ++r) s = __builtin_fma(c[r], c[r], s);
      }
      ss[j] = s;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      // lanes l, l ^ 16, l ^ 32, l ^ 48 hold the four lane groups' sums of one candidate: (g0 + g1) + (g2 + g3)
      double v = ss[j];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      const int64_t gidx = row0 + (int64_t)tile * BN + wave * 16 * NJ + j * 16 + lr;
      if (lane < 16 && gidx < Mtotal) {
        double o = (base + sgn * v) + var_add;
        if (clamp) o = (o < var_min) ? var_min : o;
        var[gidx] = o;
      }
    }
    __syncthreads();  // everybody is done with this tile's image
  }
}
}  // namespace small64

#ifndef B7_POST_NO_LAUNCHERS
namespace {
struct PostArgs {  // what one launch needs besides the kernel: S fits side by side (S = 1: the context's own fit)
  const double *Linv, *ks;
  double *var;
  double base, sgn, var_add;
  int S;
  PostBatch pb;
};

template <int NJ>
int launch_post_w4(b7_ctx *c, const PostArgs &a, int64_t row0, int64_t rows, int64_t Mtotal) {
  constexpr int lds = w4::lds_bytes<NJ>();
  B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(w4::post_kernel_w4<NJ>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(w4::post_kernel_w4<NJ>, dim3((unsigned)(rows / (64 * NJ)), a.S), dim3(256), lds, c->stream, a.Linv, a.ks,
                     c->Npad, row0, Mtotal, a.base, a.sgn, a.var_add, c->opts.var_clamp, c->opts.var_min, a.var, a.pb);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

template <int NJ, int NR>
int launch_post_tall(b7_ctx *c, const PostArgs &a, int64_t row0, int64_t rows, int64_t Mtotal) {
  using T = w4::Tall<NJ, NR>;
  auto kern = w4::post_kernel_w4t<NJ, NR>;
  B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                T::LDS_BYTES));
  hipLaunchKernelGGL(kern, dim3((unsigned)(rows / T::BN), a.S), dim3(256), T::LDS_BYTES, c->stream, a.Linv, a.ks, c->Npad, row0,
                     Mtotal, a.base, a.sgn, a.var_add, c->opts.var_clamp, c->opts.var_min, a.var, a.pb);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int launch_post_small(b7_ctx *c, const PostArgs &a, int64_t row0, int64_t rows, int64_t Mtotal) {
  B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(small64::post_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                small64::LDS_BYTES));
  // two workgroups per CU (33 KB of LDS, ~200 registers each); with S fits side by side the CUs are split between them
  const int ntiles = (int)(rows / small64::BN), S = a.S > 0 ? a.S : 1;
  int gx = (2 * c->cus + S - 1) / S;
  if (gx > ntiles) gx = ntiles;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(small64::post_small_kernel, dim3((unsigned)gx, S), dim3(256), small64::LDS_BYTES, c->stream, a.Linv, a.ks, row0,
                     Mtotal, ntiles, a.base, a.sgn, a.var_add, c->opts.var_clamp, c->opts.var_min, a.var, a.pb);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int dispatch_post(b7_ctx *c, const PostArgs &a, int64_t row0, int64_t rows, int64_t Mtotal) {
  if (rows % B7_MROWS) return b7_fail(c, B7_ERR_INVALID, "post: rows %lld not a multiple of %d", (long long)rows, B7_MROWS);
  if (c->Npad == 64) return launch_post_small(c, a, row0, rows, Mtotal);
  const bool large = rows / 256 * a.S >= c->cus;  // at least one 256-candidate workgroup per CU
  // large grids: the tall shape (n-tiles of 256 rows: half the K* bytes through the L2) when the padded N allows it
  if (c->Npad % 256 == 0 && large) return launch_post_tall<2, 16>(c, a, row0, rows, Mtotal);
  // 256 candidates per workgroup when that still gives every CU one; otherwise 128 (same arithmetic, same bits)
  if (!large) return launch_post_w4<2>(c, a, row0, rows, Mtotal);
  return launch_post_w4<4>(c, a, row0, rows, Mtotal);
}
}  // namespace

int launch_post(b7_ctx *c, const FitSet &f, const double *ks, int64_t row0, int64_t rows, int64_t Mtotal, double *var) {
  PhaseScope ps(c, "post");
  const bool blr = c->model_kind == 1;
  PostArgs a{f.Linv, ks, var, blr ? 0.0 : f.amp, blr ? 1.0 : -1.0, blr ? f.noise : (c->opts.var_with_noise ? f.noise : 0.0), 1,
             PostBatch{}};
  return dispatch_post(c, a, row0, rows, Mtotal);
}

// f's S GP fits (device scalars) over the same rows: K*_s = ks + s sks, var_s = var + s svar
int launch_post_batch(b7_ctx *c, const FitSet &f, const double *ks, int64_t sks, int64_t rows, int64_t Mtotal, double *var,
                      int64_t svar) {
  PhaseScope ps(c, "post");
  PostArgs a{f.Linv, ks, var, 0.0, -1.0, 0.0, f.S, PostBatch{}};
  a.pb.sLinv = FitSet::s_Linv(c->Npad, c->dpad);
  a.pb.sks = sks;
  a.pb.svar = svar;
  a.pb.base = f.amp_dev;
  a.pb.var_add = c->opts.var_with_noise ? f.noise_dev : nullptr;
  return dispatch_post(c, a, 0, rows, Mtotal);
}

// S Bayesian-linear heads over the SAME feature rows (b7_blr_eval_nominate_marg): Linv_s = Linv + s Npad^2, the features are
// shared (stride 0), var_s = 1/beta_s + |Linv_s z|^2 with zero_dev[S] = 0 and invbeta_dev[S] on the device
int launch_post_heads(b7_ctx *c, int S, const double *Linv, const double *feat, int64_t rows, int64_t Mtotal, double *var, int64_t svar,
                      const double *zero_dev, const double *invbeta_dev) {
  PhaseScope ps(c, "post");
  PostArgs a{Linv, feat, var, 0.0, 1.0, 0.0, S, PostBatch{}};
  a.pb.sLinv = FitSet::s_Linv(c->Npad, c->dpad);  // the heads sit in the batch slot of the fits' inverses
  a.pb.sks = 0;
  a.pb.svar = svar;
  a.pb.base = zero_dev;
  a.pb.var_add = invbeta_dev;
  return dispatch_post(c, a, 0, rows, Mtotal);
}
#endif

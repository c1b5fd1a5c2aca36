// Arithmetic that two or more translation units of libppk_hip.so need, written here once: `__device__
// __forceinline__`, or `__host__ __device__` where the host states it too (and tests/device_helpers_host.hip runs it).
// No kernel lives here.  ppk_internal.h includes this file; it also stands alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/ppk.h"

#ifndef PPK_LANES
#define PPK_LANES 64           // wavefront width on CDNA
#endif

int ppk_fail(int code, const std::string &msg);      // ppk_api.hip

// ---- condensed upper triangle: PopPUNK's row order, row k <-> (i, j), 0 <= i < j < n (src/boundary.cpp:22-31) ----
// Exact while 4 n (n - 1) is exact in a double, n <= 2^25 or so (beyond that the root's argument rounds, and from
// n ~ 2^31 it goes negative for the last rows); a matrix of 2^25 samples is 4 PB.  The tile kernels' epilogues keep
// their own row index expressions (ppk_dist_tile.inc).
__host__ __device__ __forceinline__ size_t cond_row_start(size_t i, size_t n) { return i * n - (i * (i + 1)) / 2; }
// i of row k: a double sqrt estimate, then an integer fix-up
__host__ __device__ __forceinline__ size_t cond_row_i(size_t k, size_t n) {
  const double d = sqrt((double)(4 * n * (n - 1)) - 8.0 * (double)k - 7.0);
  long long i = (long long)n - 2 - (long long)floor(d / 2.0 - 0.5);
  if (i < 0) i = 0;
  if (i > (long long)n - 2) i = (long long)n - 2;
  while (i > 0 && cond_row_start((size_t)i, n) > k) --i;
  while ((size_t)i + 2 < n && cond_row_start((size_t)i + 1, n) <= k) ++i;
  return (size_t)i;
}
__host__ __device__ __forceinline__ void cond_pair(size_t k, size_t n, int &i, int &j) {
  const size_t ii = cond_row_i(k, n);
  i = (int)ii;
  j = (int)(ii + 1 + (k - cond_row_start(ii, n)));
}
__host__ __device__ __forceinline__ size_t cond_index(size_t a, size_t b, size_t n) {   // a < b < n
  return a * n - (a * (a + 1)) / 2 + (b - a - 1);
}
// the n with n (n - 1) / 2 <= n_rows < (n + 1) n / 2
inline size_t ppk_samples_of_rows(size_t n_rows) {
  size_t n = (size_t)(0.5 * (1.0 + std::sqrt(1.0 + 8.0 * (double)n_rows)));
  while (n > 1 && n * (n - 1) / 2 > n_rows) --n;
  while ((n + 1) * n / 2 <= n_rows) ++n;
  return n;
}
// *n = the samples of a condensed matrix of n_rows rows, or PPK_ERR_ARG "<who>row count is not n(n-1)/2 ..."
inline int ppk_condensed_samples(size_t n_rows, size_t *n, const std::string &who = "",
                                 const char *expected = "self/condensed matrix") {
  *n = ppk_samples_of_rows(n_rows);
  if (*n * (*n - 1) / 2 == n_rows) return PPK_OK;
  return ppk_fail(PPK_ERR_ARG, who + "row count is not n(n-1)/2 for any n (" + expected + " expected)");
}

// ---- lower triangle: neighbour joining's order, entry e = tri(a) + b, b < a (ppk_nj.hip) ----
__host__ __device__ __forceinline__ size_t tri(size_t a) { return a * (a - 1) / 2; }   // entries before row a
// the row a of triangle entry e (tri(a) <= e < tri(a + 1))
__host__ __device__ __forceinline__ size_t row_of(size_t e) {
  size_t a = (size_t)((1.0 + sqrt(1.0 + 8.0 * (double)e)) * 0.5);
  while (a > 1 && tri(a) > e) --a;
  while (tri(a + 1) <= e) ++a;
  return a;
}
__host__ __device__ __forceinline__ size_t tidx(size_t x, size_t y) { return x > y ? tri(x) + y : tri(y) + x; }

// ---- lock-free union-find on an int parent array (ppk_network.hip, ppk_refine.hip) ----
__device__ __forceinline__ int ld_relaxed(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// root of x with path halving.  parent[x] <= x always (a root only ever links under a smaller one), so every write
// here stores an ancestor, and a racing write at worst stores a less compressed one.
__device__ __forceinline__ int uf_find(int *parent, int x) {
  while (true) {
    const int p = ld_relaxed(parent + x);
    if (p == x) return x;
    const int gp = ld_relaxed(parent + p);
    if (gp != p) st_relaxed(parent + x, gp);
    x = gp;
  }
}
// links the roots of a and b (the larger under the smaller): 1 when this call removed a component
__device__ __forceinline__ unsigned uf_union(int *parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return 0;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return 1;
  }
}
// root of x in a finished forest: plain loads, no write
__device__ __forceinline__ int uf_find_ro(const int *parent, int x) {
  for (int p = parent[x]; p != x; p = parent[x]) x = p;
  return x;
}

// ---- splitmix64's finaliser (ppk_embed.hip's generator, ppk_network.hip's source sample) ----
__host__ __device__ __forceinline__ unsigned long long ppk_fmix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// [EXT] The sampled betweenness's key of global vertex v under `seed`: a component's sample is its k
// vertices of smallest (key, v).  The rule is this project's own: cugraph's draw is its generator's and is not pinned.
__host__ __device__ __forceinline__ unsigned ppk_bt_sample_key(unsigned long long seed, unsigned long long v) {
  return (unsigned)(ppk_fmix64(seed + (v + 1) * 0x9E3779B97F4A7C15ull) >> 32);
}

// ---- order-preserving float -> uint32 keys (unsigned compare == operator< on non-NaN floats) ----
// The raw transform of the bit pattern: -0.0 sorts strictly BEFORE +0.0 (ppk_iterate.hip's sort key).
__host__ __device__ __forceinline__ unsigned ord_raw(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// The folded form: -0.0 -> +0.0 first (f + 0.0f), so the two zeros share a key and radix order equals operator<
// (ppk_square.hip, ppk_sparse.hip, ppk_mst.hip).  ord_inv gives the float back, -0.0 as +0.0.
__host__ __device__ __forceinline__ unsigned ord_of(float f) { return ord_raw(f + 0.0f); }
__host__ __device__ __forceinline__ float ord_inv(unsigned o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// ---- wave reductions ----
// The loops still written out at their call sites (ppk_boundary.hip, ppk_embed.hip, the fit's changed-label count)
// compile to other instructions through a call (profiles/shared_device/README.md); new code calls these.
// shuffle-down: the sum on lane 0, added in this fixed order (the BGMM fit's fp64 sums depend on it).  `width` is the
// shuffle's: the fit passes warpSize, the shuffle's own default -- the same lanes, but other index arithmetic than 64.
template <typename T>
__device__ __forceinline__ T wave_sum(T v, int width = PPK_LANES) {
#pragma unroll
  for (int o = PPK_LANES / 2; o > 0; o >>= 1) v += __shfl_down(v, o, width);
  return v;
}
// shuffle-xor: the sum on every lane
template <typename T>
__device__ __forceinline__ T wave_sum_all(T v) {
  for (int o = PPK_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// adds every thread's v into *out: one atomic per wave
__device__ __forceinline__ void wave_add(unsigned long long *out, unsigned long long v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

// spread the 32 bits of x to the even bit positions of a 64-bit word (wave-uniform: SALU)
__device__ __forceinline__ uint64_t spread_even(uint32_t v) {
  uint64_t x = v;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// line_dist of src/boundary.cpp:42-58: float32, un-fused, evaluated as
// ((y0*x_max) + (x0*y_max)) - (x_max*y_max)  (SURVEY.md Appendix B).
__device__ __forceinline__ float ppk_line_dist(float x0, float y0, float x_max, float y_max,
                                               int slope) {
  float side = 0.0f;
  if (slope == 2) {
    if (x_max == 0.0f || y_max == 0.0f) {
      side = __fsqrt_rn(__fadd_rn(__fmul_rn(x0, x0), __fmul_rn(y0, y0)));
    } else {
      side = __fsub_rn(__fadd_rn(__fmul_rn(y0, x_max), __fmul_rn(x0, y_max)),
                       __fmul_rn(x_max, y_max));
    }
  } else if (slope == 0) {
    side = __fsub_rn(x0, x_max);
  } else if (slope == 1) {
    side = __fsub_rn(y0, y_max);
  }
  return side;
}

// The correctly rounded float32 square root of s >= 0, as numpy's: the device sqrt (measured 1 ulp off) corrected
// against the midpoints to its neighbours, whose squares (25-bit by 25-bit) are exact in double.
__device__ __forceinline__ float sqrt_rn(float s) {
  float r = __fsqrt_rn(s);
  if (!(s > 0.0f) || isinf(s)) return r;
  const double ds = (double)s;
  for (int it = 0; it < 2; ++it) {
    const float up = nextafterf(r, INFINITY), dn = nextafterf(r, 0.0f);
    const double hi = ((double)r + (double)up) * 0.5, lo = ((double)r + (double)dn) * 0.5;
    if (hi * hi < ds) r = up;
    else if (lo * lo > ds) r = dn;
    else break;
  }
  return r;
}
// process_weights' "euclidean" (PopPUNK/network.py:646-674): float32, nothing fused, the root as numpy's
__device__ __forceinline__ float ppk_euclid(float x0, float x1) {
  return sqrt_rn(__fadd_rn(__fmul_rn(x0, x0), __fmul_rn(x1, x1)));
}

// ---- the x / scale rule and the 2-D Gaussian form ----
// BGMMFit assignment of one row (PopPUNK/bgmm.py:100-176, PopPUNK/models.py:181-187), the ONE statement every
// path uses (kernel 2, the fused tile epilogues, the DBSCAN assignment's scaling and the BGMM fit's E-step), so that
// the fused edge list equals the two-step one bit for bit.  xs = x / scale in the dtype numpy promotes to (float32 /
// float32, or float64).  The triangular solve and the quadratic form are six fused multiply-adds per component on
// the constants the host computed in double (ppk_lin_of): the pass is VALU-issue bound (profiles/bgmm/), and the
// explicit fma() is the operation count that matters -- its rounding differs from the reference's separate multiply
// and add by a few units in the last place of lpr, far below the 1e-9 the label comparison allows.
__device__ __forceinline__ double ppk_scaled_f32(float x, float scale) { return (double)__fdiv_rn(x, scale); }
// M: a model with scale_is_f64, scale_f32[2] and scale_f64[2] (ppk_bgmm; the DBSCAN assignment's AssignModel)
template <class M>
__device__ __forceinline__ void ppk_bgmm_scaled(float core, float acc, const M &m, double &xs, double &ys) {
  if (m.scale_is_f64) {
    xs = (double)core / m.scale_f64[0];
    ys = (double)acc / m.scale_f64[1];
  } else {
    xs = ppk_scaled_f32(core, m.scale_f32[0]);
    ys = ppk_scaled_f32(acc, m.scale_f32[1]);
  }
}
// the weighted log-probability of component c.  M: a model with lin[][5] and log_const[] (ppk_bgmm; the fit's FitArgs)
template <class M>
__device__ __forceinline__ double ppk_bgmm_lpr(double xs, double ys, const M &m, int c) {
  const double *l = m.lin[c];
  const double z0 = __builtin_fma(xs, l[0], l[1]);
  const double z1 = __builtin_fma(ys, l[2], __builtin_fma(z0, l[3], l[4]));
  return __builtin_fma(-0.5, __builtin_fma(z0, z0, z1 * z1), m.log_const[c]);
}
// argmax_c lpr_c, the first index on ties (np.argmax of the responsibilities, which keep the order of lpr): no
// transcendental.  KT > 0: the component count as a compile-time constant (kernel 2's instantiations for K <= 4: the
// loop unrolls and the model's constants stay in scalar registers across rows); 0: m.K at run time.  The arithmetic
// is the same statement in the same order either way.
template <int KT = 0>
__device__ __forceinline__ int ppk_bgmm_label_k(double xs, double ys, const ppk_bgmm &m) {
  double best = ppk_bgmm_lpr(xs, ys, m, 0);
  int label = 0;
  if constexpr (KT > 0) {
#pragma unroll
    for (int c = 1; c < KT; ++c) {
      const double v = ppk_bgmm_lpr(xs, ys, m, c);
      if (v > best) {
        best = v;
        label = c;
      }
    }
  } else {
    for (int c = 1; c < m.K; ++c) {
      const double v = ppk_bgmm_lpr(xs, ys, m, c);
      if (v > best) {
        best = v;
        label = c;
      }
    }
  }
  return label;
}
template <int KT = 0>
__device__ __forceinline__ int ppk_bgmm_label(float core, float acc, const ppk_bgmm &m) {
  double xs, ys;
  ppk_bgmm_scaled(core, acc, m, xs, ys);
  return ppk_bgmm_label_k<KT>(xs, ys, m);
}

// ---- the sketch rule "poppunk_amd:sketch1" (ppk_sketch.hip, tests/sketch_device_host.hip) ----
// [EXT] The hash, the bin and the densify rule below are this project's own definition of a bin sketch: pp-sketchlib
// is not in the tree, so none of the three is pinned to it.  A later pin changes these functions and nothing else.
// Codes: 0-3 = A, C, G, T; 4 = any other residue; 5 = contig break.  The seed of a code above 3 is 0: a window that
// holds one is never hashed, and the rolling form may carry such a term in and out.
__host__ __device__ __forceinline__ uint64_t ppk_sketch_seed(unsigned code) {      // ntHash's seeds [EXT: recalled]
  return code == 0 ? 0x3c8bfbb395c60474ull : code == 1 ? 0x3193c18562a02b4cull : code == 2 ? 0x20323ed082572324ull
       : code == 3 ? 0x295549f54be24456ull : 0ull;
}
__host__ __device__ __forceinline__ uint64_t ppk_sketch_seed_rc(unsigned code) {   // the complement's seed
  return code < 4 ? ppk_sketch_seed(3u - code) : 0ull;
}
__host__ __device__ __forceinline__ uint64_t ppk_rol64(uint64_t x, unsigned r) {   // rotation amounts are taken mod 64
  r &= 63u;
  return r ? (x << r) | (x >> (64u - r)) : x;
}
// min(forward, reverse), or forward alone when strand-preserved
__host__ __device__ __forceinline__ uint64_t ppk_sketch_pick(uint64_t f, uint64_t r, int strand_preserved) {
  return strand_preserved || f < r ? f : r;
}
// HASH, as defined: f = XOR_i rol(seed[s_i], k-1-i), r = XOR_i rol(seed[3-s_i], i) over the k codes at s (all < 4)
__host__ __device__ __forceinline__ uint64_t ppk_sketch_hash(const uint8_t *s, int k, int strand_preserved) {
  uint64_t f = 0, r = 0;
  for (int i = 0; i < k; ++i) {
    f ^= ppk_rol64(ppk_sketch_seed(s[i]), (unsigned)(k - 1 - i));
    r ^= ppk_rol64(ppk_sketch_seed_rc(s[i]), (unsigned)i);
  }
  return ppk_sketch_pick(f, r, strand_preserved);
}
// ... and its rolling form.  The four terms a code contributes at length k: {entering f, entering r, leaving f,
// leaving r} (the kernel keeps them in a table per code); all zero for a code above 3.
__host__ __device__ __forceinline__ void ppk_sketch_terms(unsigned code, int k, uint64_t t[4]) {
  t[0] = ppk_sketch_seed(code);
  t[1] = ppk_rol64(ppk_sketch_seed_rc(code), (unsigned)(k - 1));
  t[2] = ppk_rol64(ppk_sketch_seed(code), (unsigned)k);
  t[3] = ppk_sketch_seed_rc(code);
}
// One step: a code with terms in_f, in_r enters the window, the code k places back (out_f, out_r) leaves it.  Started
// from f = r = 0 with zero leaving terms for the first k steps, (f, r) after a step are the window's two hashes.
__host__ __device__ __forceinline__ void ppk_sketch_roll(uint64_t &f, uint64_t &r, uint64_t in_f, uint64_t in_r,
                                                         uint64_t out_f, uint64_t out_r) {
  f = ppk_rol64(f, 1) ^ out_f ^ in_f;
  r = ppk_rol64(r ^ out_r, 63) ^ in_r;
}
// BIN: floor(h * nbins / 2^64), one 64-bit multiply-high (nbins < 2^32)
__host__ __device__ __forceinline__ uint32_t ppk_sketch_bin(uint64_t h, uint32_t nbins) {
#ifdef __HIP_DEVICE_COMPILE__
  return (uint32_t)__umul64hi(h, (uint64_t)nbins);
#else
  return (uint32_t)(((unsigned __int128)h * nbins) >> 64);
#endif
}
#define PPK_SKETCH_EMPTY (~0ull)      // a bin no k-mer fell into (no hash is stored as this: see ppk_sketch_keep)
// what a bin keeps of a hash: the hash itself, except that the one value the empty mark takes is stored one lower
// (both fall into the last bin; the low bbits of the result are the bin's value)
__host__ __device__ __forceinline__ uint64_t ppk_sketch_keep(uint64_t h) { return h == PPK_SKETCH_EMPTY ? h - 1 : h; }
// DENSIFY: the bin an empty bin takes its value from -- the nearest non-empty bin above it, cyclically, in the state
// before densification.  For bin 64 * blk + lane: `mask` = the non-empty bins of its 64-bin block, `next` = the first
// non-empty bin of the blocks after it, cyclically (this block last).  Bounded and order-free: no loop.
__host__ __device__ __forceinline__ uint32_t ppk_sketch_densify_src(uint64_t mask, unsigned lane, uint32_t blk,
                                                                    uint32_t next) {
  const uint64_t above = mask >> lane;
  return above ? blk * 64u + lane + (uint32_t)__builtin_ctzll(above) : next;
}

// ---- the count filter of read samples (ppk_sketch.hip, tests/sketch_reads_device_host.hip) ----
// Which k-mers of a read sample may enter a bin: those whose PPK_SKETCH_COUNT_ROWS counters, one per row of 2^bits,
// all reach the minimum count.  [EXT] The number of rows, the remix and the default number of bits are this project's
// own: upstream's count-min table is recalled, not pinned.
#define PPK_SKETCH_COUNT_ROWS 2
#define PPK_SKETCH_COUNT_BITS_MIN 4       // what option "sketch_count_bits" may force: 4 .. 26
#define PPK_SKETCH_COUNT_BITS_MAX 26      // (two rows of 2^26 32-bit counters: 512 MiB)
// ROW INDEX [EXT]: the kept hash folded once, times an odd constant per row, cut to its top `bits` bits
__host__ __device__ __forceinline__ uint64_t ppk_sketch_count_mult(int row) {
  return row == 0 ? 0x9e3779b97f4a7c15ull : 0xc2b2ae3d27d4eb4full;
}
__host__ __device__ __forceinline__ uint32_t ppk_sketch_count_index(uint64_t h, int row, int bits) {
  return (uint32_t)(((h ^ (h >> 29)) * ppk_sketch_count_mult(row)) >> (64 - bits));
}
// DEFAULT BITS [EXT]: a function of the sample's own code count alone -- four counters per code and row, rounded up to
// a power of two, between 2^12 and 2^26 -- so that a sample is sketched the same in any company
__host__ __device__ __forceinline__ int ppk_sketch_count_bits(long long codes) {
  int b = 0;
  while (b < PPK_SKETCH_COUNT_BITS_MAX && ((long long)1 << b) < codes) ++b;
  b += 2;
  return b < 12 ? 12 : b > PPK_SKETCH_COUNT_BITS_MAX ? PPK_SKETCH_COUNT_BITS_MAX : b;
}
// LENGTH of a read sample from the four integers of its largest k: adm_occ * filled / win_occ rounded half up (0 when
// nothing was admitted).  Exact in 64 bits below 2^43 admitted occurrences; in double beyond.
__host__ __device__ __forceinline__ long long ppk_sketch_reads_length(unsigned long long adm_occ, unsigned long long filled,
                                                                      unsigned long long win_occ) {
  if (win_occ == 0 || filled == 0) return 0;
  if (adm_occ < ((unsigned long long)1 << 43) && filled < ((unsigned long long)1 << 19))
    return (long long)((2 * adm_occ * filled + win_occ) / (2 * win_occ));
  return (long long)((double)adm_occ * (double)filled / (double)win_occ + 0.5);
}

// ---- host only ----
// Lower Cholesky factor {L00, L10, L11} of [[a, b], [b, d]], as LAPACK's dpotrf (scipy.linalg.cholesky, bgmm.py:131-
// 176): false when a pivot is <= 0 or NaN
inline bool chol2(double a, double b, double d, double L[3]) {
  if (!(a > 0.0)) return false;
  const double l00 = std::sqrt(a);
  const double l10 = b / l00;
  const double r = d - l10 * l10;
  if (!(r > 0.0)) return false;
  L[0] = l00;
  L[1] = l10;
  L[2] = std::sqrt(r);
  return true;
}
// ppk_bgmm_lpr's coefficients lin[c] = {1/L00, -mu0/L00, 1/L11, -L10/L11, -mu1/L11} from the mean, L and i0 = 1/L00, i1 = 1/L11
inline void ppk_lin_of(const double mean[2], const double L[3], double i0, double i1, double lin[5]) {
  lin[0] = i0;
  lin[1] = -mean[0] * i0;
  lin[2] = i1;
  lin[3] = -L[1] * i1;
  lin[4] = -mean[1] * i1;
}
// the least r with 2^r >= n (at most 62)
inline int ceil_log2(size_t n) {
  int r = 0;
  while (r < 62 && ((size_t)1 << r) < n) ++r;
  return r;
}
